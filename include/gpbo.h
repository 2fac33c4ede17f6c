/* gpbo.h — C ABI of the MI355X (gfx950) GP-posterior + acquisition engine.
 *
 * This is the drop-in boundary (seam B3).  The reference (bayes_opt 3.3.0) is pure
 * Python and has no FFI of its own: the arithmetic on its suggest() hot path is delegated to
 * scikit-learn / SciPy.  Each entry point below replaces the call named beside it, so that a
 * maintainer binds it with ctypes behind the reference's two Python seams —
 * the sklearn estimator duck type of `optimizer._gp` and `AcquisitionFunction` subclassing.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every function returns an int status: 0 = GPBO_OK, negative = error (see enum); the message is
 *     available from gpbo_last_error(ctx) (ctx may be NULL for creation errors).
 *   - host buffers are caller-owned, C-contiguous, borrowed for the duration of the call only.
 *   - device memory is owned by the context; one HIP stream per context; a context is not
 *     thread-safe (distinct contexts may be used from distinct threads).
 *   - all matrices crossing the ABI are row-major float64 (the reference is float64 throughout,
 *     bayes_opt/target_space.py:95-96); `precision` selects the on-device arithmetic.
 *   - determinism: fixed reduction trees; arg-best ties -> lowest index; NaN -> first NaN wins
 *     (numpy argmin semantics, bayes_opt/acquisition.py:313).
 *   - environment: the library reads exactly four variables, none of which changes a result —
 *       GPBO_KSTAR_GB          k* slab workspace budget in GB (default 4)
 *       GPBO_COMM_TIMEOUT_S    deadline of a wait for a collective (default 120)
 *       GPBO_GROUP_TIMEOUT_S   deadline of a device-group job (default 300; kept >= the collective deadline + 15 s)
 *       GPBO_GROUP_HOST_MERGE  1: a device group merges its shards' records on the host instead of over RCCL
 *     (tests/test_abi.py checks the sources against this list).  Kernel A/B switches, dispatch overrides, probes and
 *     fault injection exist only in the DEBUG BUILD (-DGPBO_DEBUG, libgpbo_dbg.so), together with the entry points at
 *     the end of this header.
 */
#ifndef GPBO_H
#define GPBO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPBO_ABI_VERSION 4

enum gpbo_status {
  GPBO_OK = 0,
  GPBO_ERR_INVALID = -1,      /* bad argument (shape, enum, NULL)                    -> ValueError   */
  GPBO_ERR_HIP = -2,          /* HIP runtime failure (no device, OOM, launch error)  -> RuntimeError */
  GPBO_ERR_NOT_PD = -3,       /* K + noise*I not positive definite (see `info`)      -> LinAlgError  */
  GPBO_ERR_STATE = -4,        /* call order (predict before fit, no candidates ...)  -> RuntimeError */
  GPBO_ERR_UNSUPPORTED = -5,  /* kernel/precision/size outside the HIP path          -> NotImplementedError */
  GPBO_ERR_COMM = -6,         /* RCCL failure / missed deadline: the communicator is gone -> RuntimeError */
  GPBO_ERR_PEER = -7          /* multi-GPU: another rank's LOCAL step failed; the exchange completed and the
                                 communicators are intact — this step has no result, the next one may  -> RuntimeError */
};

/* The stationary kernels every entry point with an `int kernel` takes: RBF and the closed-form members of the Matern family
 * (nu = 2.5, 1.5, 0.5; kernels.py Matern.__call__).  Any other value is GPBO_ERR_UNSUPPORTED. */
enum gpbo_kernel { GPBO_KERNEL_RBF = 0, GPBO_KERNEL_MATERN25 = 1, GPBO_KERNEL_MATERN15 = 2, GPBO_KERNEL_MATERN05 = 3 };
/* The acquisitions every entry point with an `int acq` takes (acq_param = kappa for UCB, xi for the others).
 * GPBO_ACQ_LOG_EI is the logarithm of EI, for the late-run regime in which y_max sits above nearly every posterior mean: EI
 * itself is then decided among values of 1e-20 ... 1e-300 and is a plateau of zeros below z ~ -38.5, while its logarithm orders
 * the candidates as EI does wherever EI is representable and stays finite, with a non-zero gradient, down to z ~ -1e150.  With
 * aa = mu - y_max - xi formed left to right in fp64 and z = aa / sd:
 *   logEI = log(sd) + log h(z),  h(z) = phi(z) + z Phi(z)
 *     z > -1        log h = log(phi(z) + z Phi(z))
 *     -28 < z <= -1 log h = -z^2/2 - log(2 pi)/2 + log r,  r = 1 - sqrt(pi) t erfcx(t),  t = -z / sqrt2
 *     z <= -28      the same with r = w (1 - 3 w + 15 w^2 - ...), w = 1 / z^2: ten terms, coefficients (2k + 1)!!
 *   gradient of -logEI: -(ca dmu + cs dsd);  z > -1: ca = Phi / (sd h), cs = phi / (sd h);
 *                                            z <= -1: cs = 1 / (sd r), ca = m / (sd r), m = Phi / phi = (1 - r) / (-z)
 * Conventions: sd == 0 (a clipped variance) gives log(aa) for aa > 0, else -inf, with a zero slope; NaN mu or sd gives NaN.  The
 * selection key is the one of the other kinds, ys = -logEI: +inf is an ordinary double that sorts after every finite value, NaN
 * sorts last and the arg-best is still the first NaN.
 * Checked refusals (GPBO_ERR_INVALID): GPBO_ACQ_LOG_EI with n_constraints > 0 (gpbo_acq_argbest, its gpbo_comm_* / gpbo_group_*
 * forms, gpbo_polish_seeds: the constrained quantity would be logEI + sum_j log p_j, not a product: GPBO_ACQ_LOG_CEI below), and
 * GPBO_ACQ_LOG_EI in gpbo_evolve_mixed (the device differential evolution evaluates UCB / EI / POI only).
 *
 * GPBO_ACQ_LOG_CEI and GPBO_ACQ_LOG_FEAS are that constrained quantity and its feasibility part alone.  The constrained product
 * EI prod_j p_j underflows sooner than EI: every p_j = Phi(b) - Phi(a) is formed by subtraction, is exactly 0 a few sigma outside
 * the feasible band and cancels inside a narrow one.  The sum of logarithms stays finite and keeps its slope there; its feasibility
 * part is what to maximise while no feasible point has been observed (EI and POI have no y_max then).  The value 4 is unassigned
 * and refused as an unknown acquisition; the kinds are 5 and 6.  All arithmetic is fp64 without contraction.
 * Per constraint j the posterior is (cm, cs) from slot j + 1, a = (lb_j - cm) / cs, b = (ub_j - cm) / cs; an infinite bound gives
 * -inf / +inf without a division.
 *   log Phi(x)   x > -1: log(ndtr(x));   x <= -1: -x^2/2 + log(erfcx(-x / sqrt2)) - log 2, which does not underflow
 *   log p_j      both bounds infinite: 0 (the posterior is not looked at);  lb = -inf: log Phi(b);  ub = +inf: log Phi(-a);
 *                two-sided: a >= 0 is reflected, (a, b) -> (-b, -a), first; then
 *                  b <= 0, a <= -1  log Phi(b) + log(-expm1(log Phi(a) - log Phi(b)))       both in one tail
 *                  b <= 0, a > -1   log((erf(b / sqrt2) - erf(a / sqrt2)) / 2)              both within one sigma of the centre
 *                  a < 0 < b        log((erf(b / sqrt2) + erf(-a / sqrt2)) / 2)             straddling: two positive terms
 *                (The second of the three is a branch that moved: the expm1 form loses |log Phi(a)| Phi(a) / (phi(a) |a|) against
 *                the band's own condition number — 1.2 at a = -1, 3 at -0.3, without bound towards a = 0, where a narrow band
 *                just below the centre would lose every digit; the two erf, each of size 0.8 |x|, subtract at that condition number.)
 *   keys         GPBO_ACQ_LOG_CEI: ys = -(logEI + log p_0 + ... + log p_{n-1}), logEI as above, j ascending into one accumulator;
 *                GPBO_ACQ_LOG_FEAS: ys = -(log p_0 + ...): acq_param, y_max and slot 0's mu / sd are not read (the state checks on
 *                slot 0 stay those of the other kinds).  With n_constraints == 0 GPBO_ACQ_LOG_CEI IS GPBO_ACQ_LOG_EI, bit for bit.
 *   gradient     -(ca dmu + cs dsd) - sum_j dlog p_j,  dlog p_j = (q_b (-dcm - b dcs) - q_a (-dcm - a dcs)) / cs_j, with
 *                q_x = phi(x) / p_j formed as exp(-x^2/2 - log(2 pi)/2 - log p_j), never as the quotient (0 / 0 outside the band);
 *                an infinite bound contributes 0.  gpbo_polish_seeds forms it on the host side of the ABI (lockstep rounds; the
 *                one-launch search serves unconstrained models only, GPBO_ACQ_LOG_CEI without constraints as GPBO_ACQ_LOG_EI).
 * Conventions: cs not > 0 gives NaN (as the product form's norm(cm, cs).cdf), a == b gives -inf, a > b gives NaN, a NaN anywhere
 * gives NaN.  Selection is that of the other kinds: +inf sorts after every finite key, the first NaN wins the arg-best.
 * Accepted by gpbo_acq_argbest, gpbo_comm_acq_argbest, gpbo_group_acq_argbest and gpbo_polish_seeds.  Checked refusals
 * (GPBO_ERR_INVALID, the message names the kind): either kind in gpbo_evolve_mixed, which has no constraint arguments, and
 * GPBO_ACQ_LOG_FEAS with n_constraints == 0. */
enum gpbo_acq {
  GPBO_ACQ_UCB = 0,
  GPBO_ACQ_EI = 1,
  GPBO_ACQ_POI = 2,
  GPBO_ACQ_LOG_EI = 3,
  GPBO_ACQ_LOG_CEI = 5,  /* logEI + sum_j log p_j; n_constraints >= 0 (4 stays unassigned and refused) */
  GPBO_ACQ_LOG_FEAS = 6  /* sum_j log p_j alone; n_constraints >= 1 */
};
enum gpbo_precision { GPBO_F64 = 0, GPBO_F32 = 1 };

#define GPBO_MAX_MODELS 8   /* slot 0 = target GP, slots 1.. = constraint GPs */
#define GPBO_MAX_DIM 64
#define GPBO_MAX_SEEDS 64
#define GPBO_LML_BATCH_MAX 8 /* theta values one gpbo_lml_batch call evaluates side by side */

typedef struct gpbo_ctx gpbo_ctx;

/* ---- lifecycle -------------------------------------------------------------------------- */
int gpbo_abi_version(void);
int gpbo_device_count(int* count);
int gpbo_create(int device, gpbo_ctx** out);
int gpbo_destroy(gpbo_ctx* ctx);
const char* gpbo_last_error(const gpbo_ctx* ctx);
int gpbo_synchronize(gpbo_ctx* ctx);
/* Device properties as a JSON string (name, CUs, clocks, memory) for bench/profile headers. */
int gpbo_device_info(gpbo_ctx* ctx, char* buf, int buflen);

/* ---- fit at fixed theta ----------------------------------------------------------------- */
/* Replaces the tail of GaussianProcessRegressor.fit (sklearn/gaussian_process/_gpr.py:346-364,
 * called from bayes_opt/acquisition.py:84 and bayes_opt/constraint.py:148,151):
 *   K = k(X/ls, X/ls) + noise*I   (Matern nu = 2.5 / 1.5 / 0.5: kernels.py:1711-1738; RBF: kernels.py:1556-1565)
 *   L = cholesky(K, lower)        (_gpr.py:349)
 *   alpha = cho_solve(L, y_norm)  (_gpr.py:360-364)
 * and additionally forms W = L^-1, the operator the posterior kernel applies to k*.
 * X: (N,d) row-major; y_norm: (N,) already normalised by the caller (_gpr.py:272-277);
 * length_scale: n_ls == 1 (isotropic) or n_ls == d (anisotropic).
 * precision: GPBO_F64, or GPBO_F32 = the factorisation stays fp64 but gpbo_posterior rounds k* and W to fp32 and
 * runs the N^2-per-candidate contraction on v_mfma_f32_16x16x4_f32 (sigma accurate to ~1e-3 relative; mu stays fp64).
 * On GPBO_ERR_NOT_PD, *info = 1-based index of the first non-positive pivot (LAPACK potrf info). */
int gpbo_fit(gpbo_ctx* ctx, int slot, const double* X, const double* y_norm, int64_t N, int d,
             int kernel, const double* length_scale, int n_ls, double noise, int precision,
             int* info);

/* gpbo_fit for a scaled model  K = amplitude * k + (white + alpha) * I  — scikit-learn's ConstantKernel(amplitude) * k +
 * WhiteKernel(white) under an estimator with `alpha`.  The device fits the unit-amplitude model at noise (white + alpha) / amplitude
 * and the slot keeps amplitude and white: every later posterior of the slot (gpbo_posterior, gpbo_predict*, gpbo_polish_seeds,
 * gpbo_evolve_mixed) gives  sigma = y_std sqrt(max(amplitude (1 - |W k*|^2) + white, 0)), the mean is unchanged.  amplitude > 0,
 * white >= 0, alpha >= 0, all finite, else GPBO_ERR_INVALID.  amplitude = 1, white = 0 is gpbo_fit at noise = alpha, bit for bit.
 * gpbo_fit, gpbo_fit_begin and gpbo_lml make the slot a unit model again; gpbo_fit_append keeps the slot's amplitude and white.
 * There is no gpbo_fit_begin twin: a scaled fit is synchronous, on the context's own stream (fits pending on other slots go on). */
int gpbo_fit_scaled(gpbo_ctx* ctx, int slot, const double* X, const double* y_norm, int64_t N, int d, int kernel,
                    const double* length_scale, int n_ls, double amplitude, double white, double alpha, int precision, int* info);

/* Append n_new observations to a fitted slot at UNCHANGED kernel, length scale and noise.
 * Replaces re-running the whole fixed-theta fit (_gpr.py:346-364) on X u x_new, which is what the reference's
 * maximize() loop does every iteration (bayes_opt/bayesian_optimization.py:377-388 -> acquisition.py:79-86) and what
 * ConstantLiar's dummy refits do (acquisition.py:1130-1143).  Per new row j, O(j^2) instead of O(j^3):
 *   k = k(X[:j], x_j);  l = W k;  lambda = sqrt(1 + noise - l.l);  L[j,:] = [l, lambda];
 *   W[j,:] = [-(l^T W) / lambda, 1 / lambda]
 * then alpha = W^T (W y_norm) for ALL targets.  y_norm: the n_total = N + n_new normalised targets (the
 * normalisation of every target changes when one is added, _gpr.py:272-277).  n_new = 0 re-solves alpha for new
 * targets only (same X; the dummy-target case).  When the rows do not fit the slot's 64-row padding, or n_new > 16,
 * the factorisation is redone from the device-resident scaled inputs instead (same result as gpbo_fit).
 * On GPBO_ERR_NOT_PD the slot is left unfitted and *info = 1-based index of the failing pivot. */
int gpbo_fit_append(gpbo_ctx* ctx, int slot, const double* x_new, int64_t n_new, int d,
                    const double* y_norm, int64_t n_total, int* info);

/* gpbo_fit in two halves, for the fits that one suggest() makes back to back — the target GP and the constraint GPs
 * (bayes_opt/acquisition.py:84-86: `gp.fit(...)`, then `constraint.fit(...)` -> constraint.py:148-151, one GP per
 * constraint).  gpbo_fit_begin enqueues the whole fit of `slot` on the slot's own stream and returns; gpbo_fit_wait
 * waits for it and resolves the positive-definiteness check (GPBO_ERR_NOT_PD, *info as gpbo_fit).  A factorisation at
 * these sizes is a chain of short dependent kernels that leaves most of the chip idle, so several of them in flight
 * overlap almost perfectly (N = 8192: two fits 26.6 ms one after the other).  Between the two calls the slot must not be
 * used; every slot's result is bitwise the one gpbo_fit gives.  X and y_norm are copied with asynchronous transfers on
 * the slot's stream: they must stay alive and unchanged until gpbo_fit_wait returns (pageable memory happens to be staged
 * before the call returns, pinned or registered memory is not). */
int gpbo_fit_begin(gpbo_ctx* ctx, int slot, const double* X, const double* y_norm, int64_t N, int d, int kernel,
                   const double* length_scale, int n_ls, double noise, int precision);
int gpbo_fit_wait(gpbo_ctx* ctx, int slot, int* info);

/* Log marginal likelihood and its gradient with respect to log(length_scale) at the given theta.
 * Replaces one L-BFGS-B evaluation of GaussianProcessRegressor.log_marginal_likelihood(theta,
 * eval_gradient=True) (_gpr.py:575-652; Matern/RBF gradients kernels.py:1764-1766, 1567-1582), the inner
 * loop of the theta search in fit (_gpr.py:296-338).  grad has n_ls entries.  A non-PD kernel matrix gives
 * *lml = -inf, zero gradient and *info = pivot index (status stays GPBO_OK), as sklearn does.
 * Overwrites the slot's fit state (the slot must be re-fitted with gpbo_fit before gpbo_posterior). */
int gpbo_lml(gpbo_ctx* ctx, int slot, const double* X, const double* y_norm, int64_t N, int d,
             int kernel, const double* length_scale, int n_ls, double noise, int eval_gradient,
             double* lml, double* grad, int* info);

/* gpbo_lml for the scaled model of gpbo_fit_scaled: the log marginal likelihood of y_norm under amplitude * k + (white + alpha) * I
 * and, with eval_gradient, its gradient in [log amplitude, log length_scale ..., log white]: grad has n_ls + 2 entries.  A non-PD
 * kernel matrix gives -inf and a zero gradient, as gpbo_lml does; the slot is left unfitted, as by gpbo_lml.  Its batched twin is
 * gpbo_lml_batch_scaled below (the lanes of gpbo_lml_batch itself share one noise and one target vector). */
int gpbo_lml_scaled(gpbo_ctx* ctx, int slot, const double* X, const double* y_norm, int64_t N, int d, int kernel,
                    const double* length_scale, int n_ls, double amplitude, double white, double alpha, int eval_gradient,
                    double* lml, double* grad, int* info);

/* n_theta evaluations of gpbo_lml on the SAME (X, y_norm) at different length scales (length_scales: n_theta x n_ls,
 * row-major), in scratch models of their own ("lanes") so that the latency-bound factorisations share the device.
 * This is what the theta search's independent L-BFGS-B runs (the initial theta + n_restarts_optimizer restarts,
 * _gpr.py:296-338) need when they advance together.  Results per theta as gpbo_lml (lml[i], grad[i * n_ls ...], info[i]);
 * every lane computes exactly what gpbo_lml computes, bit for bit.  Model slots and their fits are not touched.
 * X = y_norm = NULL re-uses the inputs the previous call uploaded (same N, d) — the rounds of one theta search.
 * Below N = 2048 all lanes run through ONE sequence of ~60 launches (lane = a grid dimension of every kernel); from there
 * on each lane gets its own stream.  From the second call with the same shape a sequence is replayed as a captured hipGraph. */
int gpbo_lml_batch(gpbo_ctx* ctx, int n_theta, const double* X, const double* y_norm, int64_t N, int d, int kernel,
                   const double* length_scales, int n_ls, double noise, int eval_gradient, double* lml, double* grad,
                   int* info);

/* gpbo_lml_batch for scaled models: n_theta evaluations of gpbo_lml_scaled on the SAME (X, y_norm, alpha), lane i at
 * (amplitudes[i], length_scales[i * n_ls ...], whites[i]).  lml[i], grad[i * (n_ls + 2) ...] in [log amplitude, log length_scale ...,
 * log white] and info[i] are what gpbo_lml_scaled gives for lane i's arguments, bit for bit; a lane whose kernel matrix is not
 * positive definite gives -inf, n_ls + 2 zeros and its pivot index in info[i], the other lanes are unaffected.  Conventions of
 * gpbo_lml_batch: X = y_norm = NULL re-uses the resident inputs, pending fits are waited for, model slots are untouched, 1 ...
 * GPBO_LML_BATCH_MAX lanes, the same lane groups and captured graphs — each lane's noise (white + alpha) / amplitude and target
 * scale 1 / sqrt(amplitude) reach the kernels through the group's pinned staging words, as the length scales do, so a replayed graph
 * evaluates the call's own values.  Still refused: device groups (gpbo_group_lml_batch takes unit models only). */
int gpbo_lml_batch_scaled(gpbo_ctx* ctx, int n_theta, const double* X, const double* y_norm, int64_t N, int d, int kernel,
                          const double* length_scales, int n_ls, const double* amplitudes, const double* whites, double alpha,
                          int eval_gradient, double* lml, double* grad, int* info);

/* Parity accessors (tests): copy device state back as (N,N) row-major / (N,) float64.  For a slot of gpbo_fit_scaled K, L and
 * alpha are scikit-learn's quantities of the scaled model (c K', sqrt(c) L', alpha' / c of the unit model the device holds). */
int gpbo_get_K(gpbo_ctx* ctx, int slot, double* out);      /* kernel matrix incl. noise, full symmetric */
int gpbo_get_L(gpbo_ctx* ctx, int slot, double* out);      /* lower Cholesky factor, upper zeroed (gp.L_) */
int gpbo_get_Linv(gpbo_ctx* ctx, int slot, double* out);   /* W = L^-1, lower; of a scaled slot the UNIT model's W' = sqrt(c) L_^-1 */
int gpbo_get_alpha(gpbo_ctx* ctx, int slot, double* out);  /* gp.alpha_ */

/* ---- candidates ------------------------------------------------------------------------- */
/* Upload the candidate matrix x_tries (M,d) row-major (bayes_opt/acquisition.py:311,
 * TargetSpace.random_sample target_space.py:565-603) and keep it resident in HBM. */
int gpbo_set_candidates(gpbo_ctx* ctx, const double* Xc, int64_t M, int d);

/* Throughput mode (NOT stream-compatible with the reference): fill the resident candidate matrix with
 * M x d uniforms in [lo[t], hi[t]) from a counter-based Philox4x32-10 generator on the device, instead of
 * TargetSpace.random_sample + upload (target_space.py:565-603).  Index parity with the reference needs the
 * host RandomState stream (gpbo_set_candidates); this entry point removes the host sampling and the H2D copy. */
int gpbo_generate_candidates(gpbo_ctx* ctx, int64_t M, int d, const double* lo, const double* hi, uint64_t seed);
/* Index-parity mode: the SAME matrix TargetSpace.random_sample would return for an all-float space — column t =
 * random_state.uniform(lo[t], hi[t], M) in key order (target_space.py:593-600, parameter.py:86-87) — generated on
 * the device from the caller's MT19937 state (key[624], *pos as in RandomState.get_state()) and left resident; key
 * and *pos come back advanced by the 2*M*d outputs consumed, so RandomState.set_state() continues the reference's
 * stream.  Removes the host sampling and the upload without changing a single candidate. */
int gpbo_generate_candidates_mt19937(gpbo_ctx* ctx, int64_t M, int d, const double* lo, const double* hi,
                                     uint32_t* key, int* pos);
/* The same for rows [row_begin, row_end) only (one shard of a candidate set drawn by several GPUs from ONE stream): this
 * context keeps (row_end - row_begin) x d candidates resident.  key / pos are read only; key_out / pos_out (may be NULL)
 * receive the state after the WHOLE (M, d) draw and are written only when row_end == M. */
int gpbo_generate_candidate_rows_mt19937(gpbo_ctx* ctx, int64_t M, int d, int64_t row_begin, int64_t row_end,
                                         const double* lo, const double* hi, const uint32_t* key, int pos,
                                         uint32_t* key_out, int* pos_out);
/* MT19937 jump-ahead on the host: key_out = the 624-word block n_blocks (>= 1) after key_in, computed as
 * (x^(624 (n_blocks - 1)) mod phi)(F) applied to the state — the same polynomial route by which
 * gpbo_generate_candidates_mt19937 starts its sub-streams on the device (csrc/mt_jump.hip).  Equivalent to drawing
 * 624 * n_blocks outputs from numpy.random.RandomState and reading get_state()[1], in O(log n_blocks) polynomial products. */
int gpbo_mt19937_jump_blocks(const uint32_t key_in[624], int64_t n_blocks, uint32_t key_out[624]);
/* Trust-region mode (TuRBO; Eriksson et al. 2019, "Scalable global optimization via local Bayesian optimization"): the resident
 * candidate matrix (M, d) row-major becomes the point `centre` with a FEW coordinates of every row replaced by a point of a scrambled
 * Sobol sequence inside the box [lo, hi] — quasi-random, NOT the reference's stream.  The caller passes the sequence's tables:
 * sobol_sv (d, bits) row-major, the direction numbers after scrambling, and sobol_shift (d,), the digital shift, each word below
 * 2^bits (scipy.stats.qmc.Sobol(d, scramble=True, seed, bits): its _sv and _shift).  Row m, column t, element e = m d + t:
 *   Sobol point  g = m ^ (m >> 1);  w(m, t) = shift[t] XOR over the set bits b of g of sv[t bits + b];  u = w 2^-bits (exact);
 *                point = lo[t] + (hi[t] - lo[t]) * u, every operation rounded once (no fused multiply-add) — with lo = 0, hi = 1
 *                the matrix of points equals Sobol(...).random(M) of a fresh engine bit for bit, whatever M.
 *   mask         philox4x32_10(counter = (q_lo, q_hi, 0, 0), key = mask_key), q = e >> 2, gives four 32-bit words; element e takes
 *                word e & 3 and is PERTURBED iff word < mask_threshold (2^32: every coordinate, 0: none).
 *   fallback     a row without a perturbed coordinate gets exactly one: column (w0 d) >> 32, w0 = word 0 of
 *                philox4x32_10(counter = (m_lo, m_hi, 1, 0), key = mask_key).
 *   value        the Sobol point where perturbed, else centre[t] bit for bit.
 * lo <= centre <= hi is not required.  GPBO_ERR_INVALID, with the resident candidates and their posteriors left as they were: a NULL
 * pointer, M < 1, d outside [1, GPBO_MAX_DIM], bits outside [1, 32], M > 2^bits, mask_threshold > 2^32, a non-finite centre / lo /
 * hi, lo[t] > hi[t].  On success the context's posteriors are dropped like after gpbo_generate_candidates.  One launch; per device
 * only (no group and no communicator form). */
int gpbo_generate_candidates_trust_region(gpbo_ctx* ctx, int64_t M, int d, const double* centre, const double* lo, const double* hi,
                                          const uint32_t* sobol_sv, int bits, const uint32_t* sobol_shift, uint64_t mask_threshold,
                                          uint64_t mask_key);
/* Copy n rows (by index) of the resident candidate matrix back to the host (x_min and the seeds,
 * bayes_opt/acquisition.py:313-317); out is (n, d) row-major; out-of-range indices give NaN rows. */
int gpbo_get_candidate_rows(gpbo_ctx* ctx, const int64_t* idx, int n, double* out);

/* ---- spaces with Int / Categorical parameters (second half) -------------------------------------------
 * TargetSpace.random_sample (bayes_opt/target_space.py:593-600) draws parameter by parameter from ONE RandomState:
 * FloatParameter -> uniform (parameter.py:86-87), IntParameter / CategoricalParameter -> randint (:280-284, :360-377), whose
 * word consumption depends on the values drawn.  The matrix is therefore assembled group by group in key order, the float
 * groups on the device, the others on the host at the position the device hands back:
 *   gpbo_generate_candidate_columns_mt19937  columns [col0, col0 + ncols) = uniform(lo_t, hi_t, M) per column from (key, pos),
 *                                            which come back advanced past these 2 M ncols words;
 *   gpbo_set_candidate_columns               columns [col0, col0 + ncols) from a host array (M, ncols).
 * Every group of one matrix is written with the same (M, d_total).  gpbo_transform_candidates then applies
 * TargetSpace.kernel_transform (target_space.py:340-347) in place — kind 0: identity, 1: np.round (IntParameter,
 * parameter.py:308-320), 2: CategoricalParameter's one-hot (parameter.py:434-449, including its batch behaviour: a column
 * is set in ALL rows as soon as it is the argmax of any row) — and keeps the untransformed matrix aside:
 * gpbo_get_candidate_rows keeps returning the rows as drawn, gpbo_posterior sees the transformed ones.
 * Because of that batch behaviour a categorical group (kind 2) is a reduction over ALL M rows: the context must hold the whole
 * reference batch.  On a context that is one shard of a multi-device job (gpbo_comm_init with world_size > 1, a member of a
 * gpbo_group) a kind-2 group returns GPBO_ERR_UNSUPPORTED instead of transforming its rows differently from the reference
 * (sharded callers transform on the host, as GroupEngine does). */
int gpbo_generate_candidate_columns_mt19937(gpbo_ctx* ctx, int64_t M, int d_total, int col0, int ncols, const double* lo,
                                            const double* hi, uint32_t* key, int* pos);
int gpbo_set_candidate_columns(gpbo_ctx* ctx, const double* values, int64_t M, int d_total, int col0, int ncols);
int gpbo_transform_candidates(gpbo_ctx* ctx, int n_groups, const int* kind, const int* col0, const int* ncols);

/* ---- posterior -------------------------------------------------------------------------- */
/* Replaces GaussianProcessRegressor.predict(X, return_std=True) (_gpr.py:443-494; called from
 * bayes_opt/acquisition.py:205,216 and bayes_opt/constraint.py:200,213) for the resident
 * candidates: mu = y_std * (k* . alpha) + y_mean ; sd = sqrt(max(1 - |W k*|^2, 0) * y_std^2).
 * mu / sd may be NULL (results stay on the device for gpbo_acq_argbest). */
int gpbo_posterior(gpbo_ctx* ctx, int slot, double y_mean, double y_std, double* mu, double* sd);

/* gpbo_posterior after gpbo_fit_append, without the pass over W where none is needed (a batch of q suggestions by constant liar,
 * bayes_opt/acquisition.py:1130-1143, is one full pass and q - 1 of these).  Same outputs and conventions as gpbo_posterior: mu / sd
 * may be NULL, the results stay resident for gpbo_acq_argbest, the negative-variance flag is set whenever a variance is clipped.
 * *route (may be NULL) reports what ran: 0 = the full pass, exactly gpbo_posterior; 1 = the incremental update.
 * Route 1 needs ALL of: the slot's resident mu / sd were valid for the context's CURRENT candidate set when the last gpbo_fit_append
 * ran, and since then only gpbo_fit_append calls that took the row-append path have touched the slot (0 <= rows added in total <= 16,
 * the 64-row padding unchanged).  Everything else runs the full pass and reports 0, never a stale or mixed answer: a rebuild inside
 * append (a padding crossing, n_new > 16), gpbo_fit / gpbo_fit_scaled / gpbo_fit_begin / gpbo_lml* on the slot, any writer of the
 * candidates (gpbo_set_candidates, gpbo_generate_*, gpbo_set_candidate_columns, gpbo_transform_candidates, gpbo_predict*,
 * gpbo_polish_seeds, gpbo_evolve_mixed), a packed small-path posterior that left nothing resident.  An unfitted slot is
 * GPBO_ERR_STATE, as for every reader.  gpbo_fit_append itself still ends the resident posterior: gpbo_acq_argbest after an append
 * needs a gpbo_posterior or a gpbo_posterior_refresh first.
 * The update, for the appended rows r = N_post ... N - 1 and v_r(x) = sum_{i <= r} W[r, i] k(x, X_i) (the rows of W = L^-1 above an
 * appended row do not change, so the unit variance of every candidate drops by exactly v_r(x)^2):
 *   mu = y_std (sum_i alpha_i k(x, X_i)) + y_mean over all N rows with the new alpha (recomputed, not incremented: the targets'
 *        normalisation may have changed);
 *   sd = y_std sqrt(max((sd_old / y_std_old)^2 - amplitude sum_r v_r(x)^2, 0)), amplitude the slot's own (1 for a unit model; white
 *        is already inside sd_old).  An append with n_new = 0 refreshes mu and rescales sd.
 * One launch, one k* generation per (candidate, training point) against 1 + n_rows weight vectors: O(M N d) instead of O(M N^2).
 * fp64 whatever the slot's precision: the refreshed sigma of a GPBO_F32 slot inherits the accuracy of the fp32 pass it started from. */
int gpbo_posterior_refresh(gpbo_ctx* ctx, int slot, double y_mean, double y_std, double* mu, double* sd, int* route);

/* n_paths function draws from the slot's posterior over the resident candidates, and each draw's maximiser: Thompson sampling.
 * Replaces GaussianProcessRegressor.sample_y (_gpr.py: predict(return_cov=True), then an M x M factorisation on the host), which
 * gpbo_predict_cov bounds at M <= 16384.  A draw is conditioned pathwise (Matheron's rule; Wilson et al. 2020, "Efficiently sampling
 * functions from Gaussian process posteriors"): a random-Fourier-feature draw g_s from the prior plus a data-dependent update that
 * is exact.  With c = the slot's amplitude (1 for a unit model), xs = x / length_scale as the slot scales it, fs = sqrt(2 c / F):
 *   phi_j(x) = cos(2 pi (omega_j . xs + phase_j))         omega (F, d) in turns per unit of the LENGTH-SCALED input, phase (F,) in turns
 *   g_s(x)   = fs sum_j weights[s, j] phi_j(x)            weights (S, F)
 *   u_s      = g_s(X) + eps_s                             eps (S, N) in normalised-target units
 *   v_s      = alpha - W^T (W u_s)                        the device's unit-model alpha and W: (K + eta I)^-1 (y_n - u_s)
 *   f_s(x)   = y_std (g_s(x) + sum_i k(xs, Xs_i) v_s,i) + y_mean      the LATENT function: a scaled slot's white part is not added
 * best_idx[s] / best_val[s]: the first index of the maximum of f_s over the resident candidates (+ index_offset) and its value — the
 * rules of gpbo_acq_argbest on the key -f_s: ties -> lowest index, the first NaN wins.  values_out (S, M) path-major, or NULL.
 * The caller draws omega from the kernel's spectral density (frequencies / 2 pi), phase ~ U[0, 1), weights ~ N(0, 1) and
 * eps ~ N(0, white + alpha).  Arguments in turns keep the reduction r = t - rint(t) exact whatever the frequency (a Matern nu = 0.5
 * spectrum is Cauchy-tailed).  fp64 whatever the slot's precision; every sum has a fixed order, and path s's values are the same
 * bits whether it is evaluated alone or among 16.  Per candidate O((N + F) d) for all paths together.
 * A reader: the slot's fit, its resident mu / sd, what gpbo_posterior_refresh may still refresh, the candidates and the
 * negative-variance flag stay as they were (the context's acquisition values, gpbo_acq_argbest's ys, are overwritten).
 * GPBO_ERR_INVALID: n_paths outside [1, GPBO_MAX_PATHS], n_features outside [1, GPBO_MAX_PATH_FEATURES], a NULL input, y_std not
 * finite or not positive.  GPBO_ERR_STATE: an unfitted slot, a fit pending on the slot, no resident candidates, candidates of
 * another d.  There is no gpbo_group_* / gpbo_comm_* form. */
#define GPBO_MAX_PATHS 16
#define GPBO_MAX_PATH_FEATURES 4096
int gpbo_sample_paths(gpbo_ctx* ctx, int slot, double y_mean, double y_std, int n_paths, int n_features,
                      const double* omega, const double* phase, const double* weights, const double* eps,
                      int64_t index_offset, int64_t* best_idx, double* best_val, double* values_out);

/* Constrained Thompson sampling (the pick of SCBO; Eriksson & Poloczek 2021, "Scalable constrained Bayesian optimization"): n_paths
 * draws of the objective (slot 0) AND of each of C = n_constraints constraints (slots 1..C) over the resident candidates, and per
 * draw the best objective value among the candidates its constraint draws call feasible — where none is, the candidate of least
 * total violation.  Slots 0..C are fitted, with the candidates' d; their N, kernel kind, length scales, scale and precision may
 * differ.  y_mean / y_std (1 + C,); lb / ub (C,), not NaN, lb < ub, +-inf allowed.  The per-slot inputs of gpbo_sample_paths are
 * concatenated in slot order: omega (1 + C, F, d), phase (1 + C, F), weights (1 + C, S, F), eps = slot j's block (S, N_j), one after
 * another.  Slot j's draw c_j,s(x) is gpbo_sample_paths' f_s for that slot and those inputs (j = 0: f_s itself), the same bits.
 * Per path s and candidate x:
 *   t_j       = max(max(lb_j - c_j,s(x), c_j,s(x) - ub_j), 0) / y_std_j        a true division
 *   viol_s(x) = t_1 + ... + t_C                                                added in that order; a NaN c_j makes it NaN
 *   x is feasible for s  iff  viol_s(x) == 0  iff  lb_j <= c_j,s(x) <= ub_j for every j
 * Per path, in this order:
 *   1. a candidate with a NaN f_s or a NaN viol_s: the FIRST such index wins, best_val = best_viol = NaN, feasible_out = 0;
 *   2. else, some candidate is feasible: the first index of the maximum of f_s over the feasible ones, best_val = f_s there,
 *      best_viol = 0, feasible_out = 1;
 *   3. else: the first index of the minimum of viol_s, best_val = f_s there, best_viol = that minimum, feasible_out = 0.
 * index_offset is added to every returned index.  values_out (1 + C, S, M) or NULL: every slot's draws; viol_out (S, M) or NULL.
 * An infinite f_s is outside the contract.
 * On the device the constraints run in slot order — each pass folds its S values per candidate into one resident viol (S, M), the
 * first writing it, the later ones adding —, then the objective, whose pass reads viol and leaves the selection key (NaN / -f_s /
 * +inf) as the context's acquisition values; no (1 + C, S, M) block of values exists unless values_out asks for it.  One
 * selection over the keys, a second over viol for the rows without a feasible candidate.  fp64 whatever a slot's precision.
 * A reader, as gpbo_sample_paths: every slot's fit, the resident mu / sd, what gpbo_posterior_refresh may still refresh, the
 * candidates and the negative-variance flag stay as they were; the context's acquisition values are overwritten.
 * GPBO_ERR_INVALID: n_constraints outside [1, GPBO_MAX_MODELS - 1], n_paths or n_features out of gpbo_sample_paths' ranges, a NULL
 * among the inputs or best_idx / best_val / best_viol / feasible_out, a y_std not finite or not positive, a y_mean not finite, a
 * NaN bound, lb_j >= ub_j.  GPBO_ERR_STATE: one of slots 0..C unfitted or with a fit pending, no resident candidates, candidates or
 * a slot of another d.  There is no gpbo_group_* / gpbo_comm_* form. */
int gpbo_sample_paths_constrained(gpbo_ctx* ctx, int n_constraints, const double* y_mean, const double* y_std, const double* lb,
                                  const double* ub, int n_paths, int n_features, const double* omega, const double* phase,
                                  const double* weights, const double* eps, int64_t index_offset, int64_t* best_idx, double* best_val,
                                  double* best_viol, int* feasible_out, double* values_out, double* viol_out);

/* The draws of gpbo_sample_paths, each CLIMBED from n_starts starts to a local maximiser inside a box — Thompson sampling with the
 * local-search stage the reference's suggest() never goes without (Wilson et al. 2020 maximise their draws by gradient ascent: a
 * pathwise-conditioned draw is a closed-form function).  Arguments up to eps, and f_s itself, as gpbo_sample_paths.  With
 * xs = x / length_scale, t_j = omega_j . xs + phase_j in turns and r_i = |xs - Xs_i|:
 *   f_s(x)        = y_std (fs sum_j weights[s, j] cos(2 pi t_j) + sum_i v_s,i k(r_i)) + y_mean
 *   d f_s / d x_t = y_std (-2 pi fs sum_j weights[s, j] sin(2 pi t_j) omega_j,t + sum_i v_s,i k'(r_i) (xs_t - Xs_i,t) / r_i) / length_scale_t
 *   k'(r) / r     = -k (RBF);  -(5/3) (1 + sqrt5 r) exp(-sqrt5 r) (nu = 2.5);  -3 exp(-sqrt3 r) (nu = 1.5);  -exp(-r) / r (nu = 0.5,
 *                   and 0 at r = 0: a point exactly ON a training point takes no slope from it, the project's convention)
 * One run per (path s, start k), S x K <= 16 x 8 runs in ONE launch, a workgroup each, the evaluations — O((N + F) d), no pass over
 * W, no N limit — and the optimiser inside it: gpbo_polish_seeds' projected L-BFGS on -f_s (10 correction pairs, projected gradient
 * 1e-5, relative reduction 1e7 eps, 20 line-search steps, Armijo on the projected path; iterates always inside the box).
 * starts == NULL: the call does what gpbo_sample_paths does (the paths over the resident candidates; best_idx / best_val (S,) come
 *   back with the same bits), takes each path's n_starts best candidates by the selection's rules (ties -> lowest index, NaNs last;
 *   n_starts > M is GPBO_ERR_INVALID) and ascends from them: start_idx_out (S, K) = their indices + index_offset, column 0 =
 *   best_idx unless a NaN won it.
 * starts (S, K, d) on the host, clipped into the box: no resident candidates are needed, best_idx / best_val may be NULL,
 *   start_idx_out = -1.
 * box_lo < box_hi (d,), finite.  max_iter < 0: 15 000 iterations; max_iter == 0: no search — x_out = the clipped starts, f_out / g_out
 * = value and gradient there (one evaluation per run; status 0 where the projected gradient is already below tolerance, else 2).
 * Outputs per run: x_out (S, K, d) inside the box; f_out (S, K) = f_s(x_out), not negated; g_out (S, K, d) or NULL = d f_s / d x at
 * x_out (a non-finite component reads 0, as the optimiser took it); status_out (S, K) as gpbo_polish_seeds: 0 projected gradient below
 * tolerance, 1 relative reduction below tolerance / no further progress, 2 iteration limit or a non-finite start (x_out = the start),
 * 3 line search exhausted; n_eval_out (S, K) or NULL = evaluations, at most 4 max_iter + 64.  Every sum has a fixed order: a run's
 * bits do not depend on which other runs share the launch.  fp64 whatever the slot's precision.
 * A reader, as gpbo_sample_paths: the slot, its resident mu / sd, what gpbo_posterior_refresh may still refresh, the candidates (the
 * trial points live in the kernel; the candidate buffer is NOT borrowed, unlike gpbo_polish_seeds) and the negative-variance flag
 * stay as they were; the context's acquisition values are overwritten when starts == NULL.
 * The call returns when its longest run has stopped: the calling thread and the context's stream are held for that long (a run is
 * bounded by 4 max_iter + 64 evaluations of a few microseconds each at N + F of a few thousand; with the default 15 000 iterations a
 * pathological run is a fraction of a second) — callers that need a tighter bound pass a smaller max_iter (status 2 marks the cut).
 * GPBO_ERR_INVALID: the refusals of gpbo_sample_paths, n_starts outside [1, GPBO_MAX_PATH_STARTS], a box that is not finite or not
 * lo < hi, a NULL box / x_out / f_out / status_out / start_idx_out (and best_idx / best_val with starts == NULL).  GPBO_ERR_STATE: as
 * gpbo_sample_paths (no candidates / candidates of another d only with starts == NULL).  There is no gpbo_group_* / gpbo_comm_* form. */
#define GPBO_MAX_PATH_STARTS 8
int gpbo_ascend_paths(gpbo_ctx* ctx, int slot, double y_mean, double y_std, int n_paths, int n_features,
                      const double* omega, const double* phase, const double* weights, const double* eps,
                      int n_starts, const double* starts, const double* box_lo, const double* box_hi, int max_iter,
                      int64_t index_offset, int64_t* best_idx, double* best_val, double* x_out, double* f_out, double* g_out,
                      int* status_out, int* n_eval_out, int64_t* start_idx_out);

/* Convenience: set_candidates + posterior for a host batch (the HipGPR.predict path). */
int gpbo_predict(gpbo_ctx* ctx, int slot, const double* Xc, int64_t M, int d, double y_mean,
                 double y_std, double* mu, double* sd);

/* sklearn warns "Predicted variances smaller than 0. Setting those variances to 0." when it clips a NEGATIVE
 * variance (_gpr.py:479-485).  The device clips inside its finalize kernels; this reports (and clears) whether any
 * gpbo_posterior / gpbo_predict / gpbo_predict_grad since the last call clipped one, so the host can warn on exactly
 * sklearn's condition.  Synchronises the context's stream. */
int gpbo_take_negative_variance_flag(gpbo_ctx* ctx, int* seen);

/* Replaces GaussianProcessRegressor.predict(X, return_cov=True) (_gpr.py:443-447, 458-469; reached from
 * BayesianOptimization.predict(..., return_cov=True), bayes_opt/bayesian_optimization.py:238) for a host batch:
 * cov (M,M) row-major = (k(X, X) - V^T V) * y_std^2 with V = L^-1 K*^T formed as two MFMA GEMMs on the device (no clipping,
 * as sklearn on this branch); mu (M,) optional.  M <= 16384. */
int gpbo_predict_cov(gpbo_ctx* ctx, int slot, const double* Xc, int64_t M, int d, double y_mean, double y_std,
                     double* mu, double* cov);

/* Posterior AND its gradient in the inputs for a small host batch (M <= 256): mu, sd (M,) as gpbo_predict, and
 * dmu, dsd (M,d) = d mu / d x, d sd / d x.  One evaluation gives the local search of the reference
 * (bayes_opt/acquisition.py:365-374: scipy L-BFGS-B, which forms its gradient from d + 1 predicts by finite differences)
 * value and gradient from ONE point: u = W^T (W k*), d sd^2 / d x = -2 y_std^2 u . dk* / dx.
 * A clipped (zero) variance has zero slope.  sklearn has no counterpart; parity is against finite differences of
 * gpbo_predict / the oracle. */
int gpbo_predict_grad(gpbo_ctx* ctx, int slot, const double* Xc, int64_t M, int d, double y_mean, double y_std,
                      double* mu, double* sd, double* dmu, double* dsd);

/* The local-search stage of a suggest() as ONE call.  Replaces AcquisitionFunction._smart_minimize for an all-continuous
 * space (bayes_opt/acquisition.py:322-420: one scipy L-BFGS-B run per seed, every value a GP predict, every gradient d + 1
 * of them): all `n_seeds` runs advance in lockstep, each round is one batched evaluation of
 *   f(x) = -base_acq(mu0, sd0) [* prod_j (Phi((ub_j-mu_j)/sd_j) - Phi((lb_j-mu_j)/sd_j))]   and its gradient
 * from the posteriors of slots 0..n_constraints and their input gradients (as gpbo_predict_grad), and the optimiser
 * arithmetic (a projected L-BFGS with L-BFGS-B's stopping rule as SciPy configures it: 10 corrections, projected gradient
 * 1e-5, relative reduction 1e7 eps, 20 line-search steps, max_iter <= 0 -> 15000 iterations) runs on the host in between.
 * One model of at most 512 (padded) observations: the runs are one launch, a workgroup each, evaluations and optimiser on the
 * device — the same optimiser arithmetic, the same evaluation arithmetic, the same results (bit for bit for UCB).
 * Not the reference's iterates: parity is statistical (acquisition value at the returned point).
 * y_mean / y_std: (1 + n_constraints,) the targets' normalisation per slot; seeds (n_seeds,d), clipped into the box;
 * box_lo < box_hi (d,).  Outputs per seed: x_out (n_seeds,d) inside the box, f_out, status_out (0: projected gradient
 * below tolerance, 1: relative reduction below tolerance / no further progress, 2: iteration limit or a non-finite start —
 * SciPy's success = False), n_rounds_out (optional) = batched evaluations issued by the lockstep path, or — one model of
 * NP <= 512, where the whole stage is ONE launch (a workgroup per run) — the longest run's evaluation count; n_iter_out /
 * n_eval_out (optional, per seed) = accepted steps / objective evaluations, SciPy's nit / nfev.  The one-launch form returns when
 * its longest run has stopped: the calling thread and the context's stream are held for that long (a run is bounded by
 * 4 * max_iter + 64 evaluations of 4-40 us each; with the default max_iter = 15 000 a pathological run is ~1 s) — callers that
 * need a tighter bound pass a smaller max_iter (status 2 marks the runs it cut).  Like gpbo_predict, the call uses the context's candidate
 * buffer for its trial points: the resident candidate set is gone afterwards (fetch x_min / the seeds with
 * gpbo_get_candidate_rows first, as the reference reads x_tries before it starts its local searches, acquisition.py:313-317). */
int gpbo_polish_seeds(gpbo_ctx* ctx, int acq, double acq_param, double y_max, int n_constraints, const double* lb,
                      const double* ub, const double* y_mean, const double* y_std, const double* seeds, int n_seeds, int d,
                      const double* box_lo, const double* box_hi, int max_iter, double* x_out, double* f_out, int* status_out,
                      int* n_rounds_out, int* n_iter_out, int* n_eval_out);

/* The differential evolution of a mixed-space smart stage as ONE call.  Replaces the solver the reference runs when a space has
 * IntParameter / CategoricalParameter columns (bayes_opt/acquisition.py:375-396: DifferentialEvolutionSolver(func=acq, bounds,
 * init=population, polish=False, rng=random_state).solve(), SciPy 1.15: best1bin, mutation (0.5, 1) dithered, recombination 0.7,
 * updating 'immediate', tol 0.01, atol 0) over the objective
 *   f(x) = -base_acq(mu0, sd0) at kernel_transform(x)   (slot 0, no constraint GPs; acquisition.py:198-217, target_space.py:340-347)
 * with the walk AND its evaluations on the device: one workgroup holds the solver's state and evaluates each trial as the posterior of
 * its one point (thread = training point), launches of a bounded number of evaluations repeated until the run ends.  Every draw is
 * the one SciPy makes from the legacy RandomState whose MT19937 state is key[624] / *pos (both come back advanced, as
 * gpbo_generate_candidate_columns_mt19937's).  Column groups as gpbo_transform_candidates: kind[g] 0 float (identity), 1 int (rint),
 * 2 categorical (one-hot at the first argmax), covering columns [col0[g], col0[g] + ncols[g]) of D <= 64 exactly once.  bounds_lo /
 * bounds_hi (D,): the space's bounds; init (S, D), S in [5, 1024]: the initial population in parameter space (clipped into the box);
 * maxiter >= 1 generations.  Outputs: x_out (D,) the best member, f_out its energy, nit_out / nfev_out SciPy's nit / nfev,
 * success_out 0 when maxiter ended the run.  The energies agree with the host's to rounding, so the walk is the host solver's
 * wherever no comparison of two energies falls within it.  Slot 0 of at most 512 (padded) observations, fp64 whatever the fit's
 * precision. */
int gpbo_evolve_mixed(gpbo_ctx* ctx, int acq, double acq_param, double y_max, double y_mean, double y_std, int n_groups,
                      const int* kind, const int* col0, const int* ncols, const double* bounds_lo, const double* bounds_hi,
                      const double* init, int S, int D, int maxiter, unsigned* key, int* pos, double* x_out, double* f_out,
                      int* nit_out, int* nfev_out, int* success_out);

/* ---- acquisition + arg-best ------------------------------------------------------------- */
/* Replaces the _get_acq closure + base_acq + argmin/min/argsort[:k]
 * (bayes_opt/acquisition.py:198-217, 485, 660-661, 847-849, 312-317) and, when n_constraints > 0,
 * ConstraintModel.predict (bayes_opt/constraint.py:199-221) over the resident candidates, using
 * the posteriors left on the device by gpbo_posterior for slots 0..n_constraints:
 *   ys = -1 * base_acq(mu0, sd0) [* prod_j (Phi((ub_j-mu_j)/sd_j) - Phi((lb_j-mu_j)/sd_j))]
 * acq_param = kappa (UCB) or xi (EI/POI); y_max is ignored for UCB.
 * lb/ub: (n_constraints,), +-inf allowed (short-circuit to 0/1 as the reference does).
 * Outputs: best_idx/best_val = ys.argmin()/ys.min() (first NaN wins); seed_idx/seed_val (k_seeds,)
 * = argsort(ys)[:k] with ties -> lowest index and NaNs last; ys_out (M,) optional (NULL to skip).
 * index_offset is added to every returned index (candidate shards). */
int gpbo_acq_argbest(gpbo_ctx* ctx, int acq, double acq_param, double y_max, int n_constraints,
                     const double* lb, const double* ub, int k_seeds, int64_t index_offset,
                     int64_t* best_idx, double* best_val, int64_t* seed_idx, double* seed_val,
                     double* ys_out);

/* Max-value entropy search (MES; Wang & Jegelka 2017, "Max-value entropy search for efficient Bayesian optimization") over the
 * resident candidates: the acquisition built on the VALUE of a posterior draw's maximum, which Thompson sampling discards.  No
 * incumbent, no xi or kappa.  From slot 0's resident mu / sd (gpbo_posterior / gpbo_posterior_refresh) and n_samples = S sampled
 * maxima y_star (S,), in raw target units — the units of that mu; gpbo_ascend_paths' f_out / gpbo_sample_paths' best_val supply them:
 *   gamma_s(x) = (y_star[s] - mu(x)) / sd(x)
 *   a(x)       = 1/S sum_s h(gamma_s(x)),      h(g) = g phi(g) / (2 Phi(g)) - log Phi(g)
 *   ys         = -a                            the reduction of the maximum's entropy from observing x, negated
 * h >= 0 is strictly decreasing, so ys <= 0.  It is evaluated over three ranges:
 *   -1 < g <= 0   as written (Phi, phi as gpbo_acq_argbest's EI evaluates them);
 *   g > 0         through the complement q = Phi(-g) = erfc(g / sqrt2) / 2: h = g phi / (2 (1 - q)) - log1p(-q) — log of a Phi rounded
 *                 next to 1 is 0.2 % off at g = 8 and 0.9 % at g = 15; h is subnormal above g ~ 37 and exactly 0 from g = 40 on;
 *   g <= -1       the two halves each grow like g^2 / 2 and cancel: with r = 1 + g Phi / phi as GPBO_ACQ_LOG_EI forms it (erfcx down
 *                 to g = -28, the asymptotic series below) and the lower-tail Mills ratio m = (1 - r) / (-g) = Phi / phi,
 *                 h = g r / (2 m) + log(2 pi) / 2 - log m, which grows like log|g| (below g = -1e150 its limit
 *                 -1/2 + log(2 pi) / 2 + log(-g) is taken; +inf at -inf).
 * Relative error against a (1 + g^2) eps model: the division that made g carries that much.
 * Conventions: a clipped variance (sd == 0) gives a = 0 — the point carries no information — unless mu is NaN; a NaN mu or sd gives
 * NaN, and the selection's "first NaN wins" rule applies.  The sum over s runs s = 0 .. S - 1 in that order, then one division by S:
 * a candidate's bits depend neither on M nor on the other candidates.  fp64 whatever the slot's precision.
 * Outputs as gpbo_acq_argbest on the key ys: best_idx / best_val = argmin / min (first NaN wins); seed_idx / seed_val (k_seeds,) =
 * argsort(ys)[:k] with ties -> lowest index and NaNs last (k_seeds may be 0, seed_* NULL); ys_out (M,) optional; index_offset is
 * added to every returned index.
 * A reader: the slot's fit, its resident mu / sd, what gpbo_posterior_refresh may still refresh, the candidates and the
 * negative-variance flag stay as they were; only the context's acquisition values (gpbo_acq_argbest's ys) are overwritten.
 * GPBO_ERR_INVALID: n_samples outside [1, GPBO_MAX_MES_SAMPLES], a NULL or non-finite y_star, k_seeds outside [0, GPBO_MAX_SEEDS],
 * a NULL best_idx / best_val (seed_idx / seed_val with k_seeds > 0).  GPBO_ERR_STATE: as gpbo_acq_argbest — slot 0 unfitted, no
 * candidates, no resident posterior for them.  There is no gpbo_group_* / gpbo_comm_* form. */
#define GPBO_MAX_MES_SAMPLES 64
int gpbo_mes_argbest(gpbo_ctx* ctx, int n_samples, const double* y_star, int k_seeds, int64_t index_offset,
                     int64_t* best_idx, double* best_val, int64_t* seed_idx, double* seed_val, double* ys_out);

/* Knowledge gradient (KG; Frazier, Powell & Dayanik 2009, "The knowledge-gradient policy for correlated normal beliefs"; Scott,
 * Frazier & Powell 2011 for continuous parameters) over the resident candidates, in its discrete form: a candidate is scored by how
 * much OBSERVING it would raise the maximum of the posterior MEAN over itself and n_points = J reference points — the look-ahead
 * acquisition for noisy objectives, where EI's incumbent is itself a noisy number.  From slot 0's resident mu / sd (y_mean / y_std:
 * those of the pass that left them; y_std must be the recorded one) and `points` (J, d), host, in parameter space (scaled by the
 * slot's length scales on the device).  c, w: the slot's amplitude and white (1, 0 for a unit model); eta: the diagonal noise of
 * the slot's unit model; lambda = c eta the observation noise in normalised-target units (white + alpha of gpbo_fit_scaled, `noise`
 * of gpbo_fit).  Per candidate x:
 *   B_j      = W^T (W k*(a_j))                                   the unit model's K'^-1 k*(a_j), once per point
 *   cov_j(x) = c (k(x, a_j) - sum_i k(x, X_i) B_j,i)             latent posterior covariance, normalised units
 *   mu_j     = y_std (sum_i alpha_i k(a_j, X_i)) + y_mean        posterior mean at a_j (mu_points_out, (J,) or NULL)
 *   v(x)     = (sd(x) / y_std)^2                                 resident; includes a scaled slot's white
 *   den(x)   = sqrt(v(x) + lambda - w)                           sd of the OBSERVATION at x
 *   lines    : (a_0, b_0) = (mu(x), y_std max(v(x) - w, 0) / den(x)),   (a_j, b_j) = (mu_j, y_std cov_j(x) / den(x)), j = 1 .. J
 *   KG(x)    = E_Z[max_j (a_j + b_j Z)] - max_j a_j >= 0,  Z ~ N(0, 1);      ys = -KG
 * evaluated exactly by Frazier's algorithm: the lines ordered by (slope, intercept), among equal slopes the largest intercept kept,
 * the upper envelope with its breakpoints c_1 < ... < c_{n-1}, KG = sum_i (b_{i+1} - b_i) f(-|c_i|), f(z) = phi(z) + z Phi(z) (Phi,
 * phi as gpbo_acq_argbest's EI evaluates them).  The lines are ORDERED first, so the result does not depend on the order in which
 * equal lines arrive.  O(N d + N J) per candidate, against the O(N^2) of the posterior pass that left mu / sd.
 * Conventions: den(x) == 0 gives KG = 0 (nothing is learned); a NaN mu(x) or sd(x), or a line with a NaN or infinite entry, gives
 * NaN, and the selection's "first NaN wins" rule applies.  Every sum has a fixed order: a candidate's bits depend neither on M nor
 * on the other candidates.  fp64 whatever the slot's precision.
 * Outputs, selection and index_offset exactly as gpbo_mes_argbest, on the key ys.
 * A reader: the slot's fit, its resident mu / sd, what gpbo_posterior_refresh may still refresh, the candidates and the
 * negative-variance flag stay as they were; only the context's acquisition values are overwritten.  The points are staged in a
 * workspace of the call's own (the candidate buffer is not borrowed).
 * GPBO_ERR_INVALID: n_points outside [1, GPBO_MAX_KG_POINTS], d not the slot's, NULL or non-finite points, k_seeds outside
 * [0, GPBO_MAX_SEEDS], a NULL best_idx / best_val (seed_idx / seed_val with k_seeds > 0), y_mean not finite, y_std not finite, not
 * positive or not the one the resident posterior was scaled with.  GPBO_ERR_STATE: slot 0 unfitted or with a fit pending, no
 * candidates, no resident posterior for them.  There is no gpbo_group_* / gpbo_comm_* form. */
#define GPBO_MAX_KG_POINTS 64
int gpbo_kg_argbest(gpbo_ctx* ctx, const double* points, int n_points, int d, double y_mean, double y_std, int k_seeds,
                    int64_t index_offset, int64_t* best_idx, double* best_val, int64_t* seed_idx, double* seed_val,
                    double* ys_out, double* mu_points_out);

/* Expected hypervolume improvement (EHVI; Emmerich, Giannakoglou & Naujoks 2006; the box form of Yang, Emmerich, Deutz & Bäck 2019)
 * over the resident candidates: the acquisition for m = n_objectives objectives at once, ALL MAXIMISED, raw target units.  Objective j
 * is slot j (0 .. m - 1); each slot's resident mu / sd (gpbo_posterior / gpbo_posterior_refresh) gives an independent posterior
 * Y_j ~ N(mu_j(x), sd_j(x)^2).  For a reference point r and a non-dominated front P strictly above r, the region above r that P does
 * not dominate is cut into K = n_cells disjoint boxes [l_k, u_k); every bound along objective j is an entry of objective j's level
 * list: r_j, the distinct front values, +inf last.
 *   levels   (m, GPBO_MAX_EHVI_LEVELS) row-major; row j holds n_levels[j] strictly increasing values, the last +inf, the others finite
 *   cell_lo / cell_hi   (K, m) level indices, lo < hi < n_levels[j].  The device does NOT check that the boxes are disjoint or tile
 *            anything: that is host policy (bayesianoptimization_amd/multiobjective.py: box_decomposition)
 *   g_j(a)  = E[(Y_j - a)^+] = sd_j f((mu_j - a) / sd_j),   f(z) = phi(z) + z Phi(z),   g_j(+inf) = 0
 *   EHVI(x) = sum_k prod_j (g_j(l_kj) - g_j(u_kj))            each factor is E[clip(Y_j, l, u) - l] >= 0
 *   ys      = -EHVI                                           so ys <= 0
 * f is evaluated over two ranges: z > -1 as written (Phi, phi as gpbo_acq_argbest's EI evaluates them); z <= -1 as phi(z) r(z),
 * r = 1 + z Phi / phi as GPBO_ACQ_LOG_EI forms it (erfcx down to z = -28, the asymptotic series below) — a candidate far below the
 * front keeps a relatively accurate, correctly ordered value instead of a cancelled one.  Where phi underflows (z < ~ -38.6) f is 0.
 * Every g_j(level) is evaluated once per candidate, not once per box.
 * Conventions: sd_j == 0 gives g_j(a) = max(mu_j - a, 0) — with every sd zero the value is the hypervolume improvement of the mean;
 * a NaN mu or sd in ANY objective gives NaN, and the selection's "first NaN wins" rule applies.  fp64 whatever a slot's precision.
 * The order of the sum.  With T = m * max_j n_levels[j], a workgroup serves C candidates and splits the boxes over G = 512 / C groups:
 *   T <= 80: C = 256, G = 2      T <= 160: C = 128, G = 4      T <= 320: C = 64, G = 8      T > 320: C = 32, G = 16
 * (the largest C whose tables T * C * 8 bytes fit 160 KiB of LDS; m = 2: max n_levels 40 | 41, 80 | 81; m = 3: 26 | 27, 53 | 54,
 * 106 | 107).  Group g sums the boxes [g P, min(K, (g + 1) P)), P = ceil(K / G), k ascending into one accumulator from 0; the G sums
 * are then added g = 0 .. G - 1 in that order.  C, G and P depend on m, the level counts and K only: a candidate's bits depend
 * neither on M, nor on the launch geometry, nor on the other candidates.
 * Outputs, selection and index_offset exactly as gpbo_mes_argbest, on the key ys.
 * A reader: the slots' fits, their resident mu / sd, what gpbo_posterior_refresh may still refresh, the candidates and the
 * negative-variance flag stay as they were; only the context's acquisition values are overwritten.  Levels and boxes are staged in a
 * workspace of the call's own.
 * GPBO_ERR_INVALID: n_objectives outside [2, GPBO_MAX_EHVI_OBJECTIVES]; a NULL n_levels / levels / cell_lo / cell_hi; a level count
 * outside [2, GPBO_MAX_EHVI_LEVELS]; levels not strictly increasing, a non-final level not finite, a final level other than +inf;
 * n_cells outside [1, GPBO_MAX_EHVI_CELLS]; a box index >= n_levels[j] or lo >= hi; k_seeds outside [0, GPBO_MAX_SEEDS]; a NULL
 * best_idx / best_val (seed_idx / seed_val with k_seeds > 0).  GPBO_ERR_STATE: one of the slots 0 .. m - 1 unfitted or with a fit
 * pending, no candidates, a slot without a resident posterior for them.  There is no gpbo_group_* / gpbo_comm_* form. */
#define GPBO_MAX_EHVI_OBJECTIVES 3
#define GPBO_MAX_EHVI_LEVELS     130      /* r_j, up to 128 distinct front values, +inf */
#define GPBO_MAX_EHVI_CELLS      16641    /* 129^2: the grid decomposition's worst case at m = 3 */
int gpbo_ehvi_argbest(gpbo_ctx* ctx, int n_objectives, const int* n_levels, const double* levels,
                      int64_t n_cells, const uint8_t* cell_lo, const uint8_t* cell_hi,
                      int k_seeds, int64_t index_offset, int64_t* best_idx, double* best_val,
                      int64_t* seed_idx, double* seed_val, double* ys_out);

/* Batch noisy expected improvement, built greedily over the resident candidates from joint posterior draws (qNEI: Letham, Karrer,
 * Ottoni & Bakshy 2019, "Constrained Bayesian optimization with noisy experiments"; the Monte-Carlo qEI of Wilson, Hutter &
 * Deisenroth 2018).  T = n_groups * n_paths draws f_t of the LATENT function, each with an incumbent m_t of its own; a candidate is
 * worth the mean over the draws of how far it lifts the incumbent; after a pick every draw's incumbent absorbs the draw's value
 * there, so the next pick is scored jointly with the earlier ones — no made-up observation, no refit.  Raw target units.
 * The draws.  G = n_groups groups of S = n_paths draws; a group shares its F = n_features features.  The inputs are the per-group
 * inputs of gpbo_sample_paths concatenated in group order: omega (G, F, d), phase (G, F), weights (G, S, F), eps (G, S, N).  Draw
 * t = g S + s is gpbo_sample_paths' f_s for group g's inputs, the same bits (the same kernels write row t of a resident (T, M) block).
 * values_out (T, M) draw-major, or NULL.
 * The incumbents.  noisy != 0: m_t = max_i f_t(X_i) over the N training points, the draw evaluated there by the evaluator the
 * candidates get (y_best is not read) — the best LATENT value among the observations, per draw, instead of one noisy measurement.
 * noisy == 0: m_t = y_best (finite) for every t: plain Monte-Carlo qEI.  Then m_t = max(m_t, f_t(p)) over the n_pending rows of
 * `pending` (P, d; host, parameter space — points suggested but not yet observed; scaled by the slot's length scales on the
 * device; n_pending = 0 with pending NULL is allowed).  The maxima are fmax folds in index order: a NaN value is dropped (m_t is NaN
 * only when every value is), and a zero's sign reaches no key, so the wave that folds a draw's values lane by lane gives the value
 * the index-order fold gives.  baseline_out (T,) = m_t before the first pick.
 * The greedy steps j = 0 .. q - 1, over the resident candidates x:
 *   term_t(x) = f_t(x) - m_t  where that is > 0;  0 where it is <= 0 (or m_t is NaN);  NaN where f_t(x) is NaN
 *   key_j(x)  = -((term_0 + term_1 + ... + term_{T-1}) / T)      added in that order into one accumulator from 0, ONE true division;
 *               +inf for a candidate picked in an earlier step
 * The pick is the selection's one-pick answer over key_j (gpbo_acq_argbest's rules: the first NaN wins, else the least key, ties
 * to the lowest index).  pick_idx[j] = its index + index_offset, pick_gain[j] = -key_j there (NaN for a NaN pick).  Then
 * m_t = fmax(m_t, f_t(pick)) for every t; a NaN value leaves m_t as it is.  Once every draw's maximum over the candidates is
 * absorbed the best gain is exactly 0 and the rule hands out the lowest unpicked index.  No multiply-add appears anywhere in a key;
 * a candidate's key bits depend neither on M, nor on the launch geometry, nor on the other candidates.  keys_out (q, M) or NULL:
 * every step's keys, masks included (a debugging aid: it adds one blocking copy per step).
 * On the device: per group one launch_path_weights and passes of path_eval_kernel over the candidates, the training points and the
 * pending points, straight into the call's workspace; one wave per draw folds the incumbent; per step qnei_score_kernel (thread =
 * candidate(s), a pure stream of the 8 T M bytes of the block, the m_t read from LDS as broadcasts) writes key_j as the context's
 * acquisition values, the selection launches pick, and qnei_update_kernel reads the pick from the selection's device record, files
 * {gain, index}, marks the mask and updates the m_t from the pick's column.  All q steps are enqueued on the context's stream; the
 * q records, baseline_out and values_out cross once, behind ONE synchronisation.  fp64 whatever the slot's precision.
 * Workspace: the context's own, 8 T M bytes for the block (2 GiB at T = 256 and M = 2^20) + 8 T (N + P) + O(M / 8 + P d) bytes; it is
 * grown on demand and kept; an allocation that fails is GPBO_ERR_HIP.
 * A reader, as gpbo_sample_paths: the slot's fit, its resident mu / sd, what gpbo_posterior_refresh may still refresh, the
 * candidates and the negative-variance flag stay as they were; the context's acquisition values are overwritten.
 * GPBO_ERR_INVALID: n_groups outside [1, GPBO_MAX_QNEI_GROUPS]; n_paths outside [1, GPBO_MAX_PATHS] or n_features outside
 * [1, GPBO_MAX_PATH_FEATURES]; a NULL omega / phase / weights / eps / pick_idx / pick_gain / baseline_out; y_std not finite or not
 * positive, y_mean not finite; noisy == 0 with a y_best that is not finite; n_pending outside [0, GPBO_MAX_QNEI_POINTS], n_pending > 0
 * with a NULL or non-finite pending, d not the slot's; q outside [1, GPBO_MAX_SEEDS], q > M.  GPBO_ERR_STATE: an unfitted slot, a fit
 * pending on the slot, no resident candidates, candidates of another d.  There is no gpbo_group_* / gpbo_comm_* form. */
#define GPBO_MAX_QNEI_GROUPS 16      /* T = n_groups * n_paths <= 256 draws */
#define GPBO_MAX_QNEI_POINTS 64      /* pending points */
int gpbo_qnei_greedy(gpbo_ctx* ctx, int slot, double y_mean, double y_std,
                     int n_groups, int n_paths, int n_features,
                     const double* omega, const double* phase, const double* weights, const double* eps,
                     int noisy, double y_best, const double* pending, int n_pending, int d,
                     int q, int64_t index_offset,
                     int64_t* pick_idx, double* pick_gain, double* baseline_out,
                     double* values_out, double* keys_out);

/* Batch noisy expected hypervolume improvement for m = 2 objectives, built greedily over the resident candidates from joint
 * posterior draws (qNEHVI: Daulton, Balandat & Bakshy 2021, "Parallel Bayesian optimization of multiple noisy objectives with
 * expected hypervolume improvement", in its greedy, cached-draws form).  Every draw carries a Pareto front of its own — the draw's
 * values at the observed and the pending points, not the noisy readings —, a candidate is worth the mean over the draws of the
 * hypervolume it adds to the draw's front, and after a pick every draw's front absorbs the draw's values there: the next pick is
 * scored jointly with the earlier ones, no observation is made up, nothing is refitted.  m = 3 is not served (and not approximated).
 * Objectives and draws.  Objective j is slot j, j = 0, 1; both are MAXIMISED, raw target units; y_mean / y_std (2,) per objective.
 * Both slots are fitted with the candidates' d; N, kernel kind, length scales, scale and precision may differ.  T = G S draws per
 * objective, G = n_groups <= GPBO_MAX_QNEI_GROUPS, S = n_paths <= GPBO_MAX_PATHS, F = n_features.  The per-slot inputs of
 * gpbo_qnei_greedy are concatenated in slot order: omega (2, G, F, d), phase (2, G, F), weights (2, G, S, F), eps = slot 0's
 * (G, S, N_0) block, then slot 1's (G, S, N_1).  Draw t = g S + s of objective j is gpbo_sample_paths' f_s for slot j and group g's
 * inputs, the same bits (the same kernels write a resident (2, T, M) block); draw t of objective 0 and draw t of objective 1 are
 * joint draw t (independent posteriors, as in gpbo_ehvi_argbest).
 * Fronts.  base (n_base, d; host, parameter space): the observed points, then the pending ones; n_base = 0 with NULL is allowed.
 * Each slot scales it by its own length scales on the device; b_t,i = (f0_t(base_i), f1_t(base_i)) by the evaluator the candidates
 * get.  ref (2,) finite.  The front P_t of draw t: the DISTINCT b_t,i strictly above ref in both objectives, without a NaN, that no
 * other such point dominates (>= in both, > in one); stored by objective 0 DESCENDING, so objective 1 strictly ascends:
 * (a_1, c_1) ... (a_n, c_n).  With a_0 = +inf, a_{n+1} = ref_0, c_0 = ref_1, strip k = 0 .. n is (a_{k+1}, a_k] x (c_k, +inf).
 * The greedy steps j = 0 .. q - 1, for candidate x with (f0, f1) = joint draw t at x:
 *   w_k      = min(f0, a_k) - a_{k+1}   where that is > 0, else 0
 *   h_k      = f1 - c_k                 where that is > 0, else 0
 *   HVI_t(x) = w_0 h_0 + w_1 h_1 + ... + w_n h_n        k ascending into one accumulator from 0, one rounded product per term, NO
 *              fused multiply-add;  NaN if f0 or f1 is NaN
 *   key_j(x) = -((HVI_0 + ... + HVI_{T-1}) / T)         t ascending into one accumulator from 0, ONE true division;
 *              +inf for a candidate picked in an earlier step
 * Every term is >= +0.  An infinite draw value is outside the contract.  The pick is gpbo_acq_argbest's on key_j: the first NaN
 * wins, else the least key, ties to the lowest index.  pick_idx[j] = its index + index_offset, pick_gain[j] = -key_j there (NaN for
 * a NaN pick).  A candidate's key bits depend neither on M, nor on the launch geometry, nor on the other candidates.
 * Update.  After a pick every draw's front absorbs y = (f0_t(pick), f1_t(pick)): P_t is unchanged if y has a NaN, is not strictly
 * above ref in both objectives, or is dominated by or equal to a point of P_t; otherwise the points y dominates leave and y enters
 * in its sorted place.
 * Overflow.  A front of more than GPBO_MAX_QNEHVI_FRONT points, at the build or after an insertion, sets a device flag; the call
 * then returns GPBO_ERR_UNSUPPORTED behind its one synchronisation, the message names the (lowest such) draw, the outputs are
 * unspecified, the context stays usable.  A front is never thinned.
 * Outputs.  front_size_out (2, T) ints and fronts_out (2, T, GPBO_MAX_QNEHVI_FRONT, 2), either may be NULL: block [0] before the
 * first pick, block [1] after the last; rows past a front's size are unspecified.  values_out (2, T, M) or NULL; base_values_out
 * (2, T, n_base) or NULL; keys_out (q, M) or NULL (a debugging aid: one copy per step).
 * On the device: per slot the candidates' and the base points' scaling, per group one launch_path_weights and passes of
 * path_eval_kernel over both; qnehvi_front_kernel (a workgroup per draw) builds P_t point by point from the right, each point the
 * lexicographic maximum of the pairs above the last point's objective 1; per step qnehvi_score_kernel (thread = candidate(s), a
 * stream of the 16 T M bytes of the block, the fronts staged in LDS as strips (a_{k+1}, c_k), 16 draws at a time, and read back as
 * wave-wide broadcasts) writes key_j as the context's acquisition values, the selection picks, and qnehvi_update_kernel reads the
 * pick from the selection's device record, files {gain, index}, marks the mask and applies the update rule per draw.  All q steps
 * are enqueued on the context's stream; everything crosses behind ONE synchronisation.  fp64 whatever the slots' precision.
 * Workspace: the context's own, 16 T M bytes for the block (4 GiB at T = 256 and M = 2^20) + 16 T n_base + 4 KiB per draw for the
 * fronts + O(M / 8 + n_base d) bytes; grown on demand and kept; an allocation that fails is GPBO_ERR_HIP.
 * A reader, as gpbo_sample_paths: the fits, the resident mu / sd, what gpbo_posterior_refresh may still refresh, the candidates
 * and the negative-variance flag stay as they were; the context's acquisition values are overwritten.
 * GPBO_ERR_INVALID: n_groups outside [1, GPBO_MAX_QNEI_GROUPS]; n_paths outside [1, GPBO_MAX_PATHS] or n_features outside
 * [1, GPBO_MAX_PATH_FEATURES]; a NULL y_mean / y_std / omega / phase / weights / eps / ref / pick_idx / pick_gain; a y_std not finite
 * or not positive, a y_mean or ref not finite; n_base outside [0, GPBO_MAX_QNEHVI_BASE], n_base > 0 with a NULL or non-finite base;
 * d not the slots'; q outside [1, GPBO_MAX_SEEDS], q > M.  GPBO_ERR_STATE: slot 0 or 1 unfitted or with a fit pending, no resident
 * candidates, candidates or a slot of another d.  There is no gpbo_group_* / gpbo_comm_* form.
 * (The symbol is spelled qnhvi — q, noisy, hypervolume improvement —: a product symbol that contains "ehvi" would read as a second
 * form of gpbo_ehvi_argbest, which has none.  The limits, the debug entry points and the Python names keep the usual "qnehvi".) */
#define GPBO_MAX_QNEHVI_FRONT 128      /* points of one draw's front */
#define GPBO_MAX_QNEHVI_BASE  16384    /* observed + pending points */
int gpbo_qnhvi_greedy(gpbo_ctx* ctx, const double* y_mean, const double* y_std,
                       int n_groups, int n_paths, int n_features,
                       const double* omega, const double* phase, const double* weights, const double* eps,
                       const double* ref, const double* base, int n_base, int d,
                       int q, int64_t index_offset,
                       int64_t* pick_idx, double* pick_gain,
                       int* front_size_out, double* fronts_out,
                       double* values_out, double* base_values_out, double* keys_out);

/* ---- timing (HIP events on the context stream) ------------------------------------------ */
/* Milliseconds spent in the last call's kernels: [0] fit total, [1] posterior main kernel,
 * [2] posterior finalize, [3] acquisition + arg-best, [4] kmat assembly, [5] cholesky, [6] trtri. */
int gpbo_last_timings(gpbo_ctx* ctx, float* ms, int n);
/* on = 0: the calls stop recording their event pairs (gpbo_last_timings then answers -1 everywhere); on = 1 (the state of a
 * new context): they record them.  A record is a marker packet on the stream — a step of BASELINE config 1 (0.12 ms: fit + posterior +
 * acquisition + arg-best) carries eight of them — so callers that never read the timings (accelerate(), bayes_opt's loop) switch
 * them off.  No result depends on it. */
int gpbo_set_timing(gpbo_ctx* ctx, int on);

/* ---- multi-GPU (RCCL over xGMI) --------------------------------------------------------- */
/* The candidate rows are independent (sklearn _gpr.py:443-494 is row-wise; bayes_opt/acquisition.py:312-317 needs only
 * the global argmin and the k best), so the candidate matrix is block-partitioned in index order, every GPU fits the
 * same GP redundantly (deterministic -> identical L) and evaluates its block, and ONE exchange — ncclAllGather of each
 * shard's 1 + k (value, global index) records, 16 bytes each, produced on the device — precedes an identical merge
 * on every rank: first NaN wins the arg-best, otherwise lexicographic (value, index); seeds = the k smallest.
 *
 * (a) one process per GPU.  rank 0 calls gpbo_comm_unique_id and ships the 128 bytes to its peers through any host
 * channel; every rank calls gpbo_comm_init; gpbo_comm_acq_argbest is gpbo_acq_argbest over the union of all shards
 * (index_offset = first global row of this rank's shard); outputs are identical on every rank. */
int gpbo_comm_unique_id(char id[128]);
int gpbo_comm_init(gpbo_ctx* ctx, const char id[128], int world_size, int rank);
int gpbo_comm_acq_argbest(gpbo_ctx* ctx, int acq, double acq_param, double y_max, int n_constraints,
                          const double* lb, const double* ub, int k_seeds, int64_t index_offset,
                          int64_t* best_idx, double* best_val, int64_t* seed_idx, double* seed_val,
                          double* ys_out /* this rank's shard, (M_local,) or NULL */);
/* Host records in, gathered host records out (n_records per rank, rank-major): the bare exchange, for callers that
 * select on the host. */
int gpbo_comm_allgather_best(gpbo_ctx* ctx, const double* vals, const int64_t* idxs, int n_records,
                             double* all_vals, int64_t* all_idxs);
/* Drain this rank's stream, then *value = max over ranks (ncclAllReduce): barrier + max-over-ranks timing. */
int gpbo_comm_allreduce_max(gpbo_ctx* ctx, double* value);
int gpbo_comm_destroy(gpbo_ctx* ctx);

/* (b) one process, G GPUs — what sits behind BayesianOptimization.suggest(), which is a single Python process
 * (bayes_opt/bayesian_optimization.py:323-333).  gpbo_group_create opens one context per entry of `devices`
 * (ncclCommInitAll) and one host thread per context; every gpbo_group_* call runs its per-device part on all devices
 * concurrently and returns when all are done.  Listing a device more than once gives VIRTUAL ranks (several shards on
 * one GPU, records merged on the host without RCCL): the single-GPU rehearsal of the sharded path.
 * gpbo_group_collective: "rccl-allgather" or "host-merge(virtual ranks)". */
typedef struct gpbo_group gpbo_group;
int gpbo_group_create(int n_dev, const int* devices, gpbo_group** out);
int gpbo_group_destroy(gpbo_group* grp);
int gpbo_group_size(const gpbo_group* grp);
gpbo_ctx* gpbo_group_ctx(gpbo_group* grp, int rank);          /* borrowed: parity accessors, timings, small predicts */
const char* gpbo_group_collective(const gpbo_group* grp);
const char* gpbo_group_last_error(const gpbo_group* grp);
int gpbo_group_synchronize(gpbo_group* grp);
/* gpbo_fit / gpbo_fit_append on every device (replicated model). */
int gpbo_group_fit(gpbo_group* grp, int slot, const double* X, const double* y_norm, int64_t N, int d, int kernel,
                   const double* length_scale, int n_ls, double noise, int precision, int* info);
int gpbo_group_fit_append(gpbo_group* grp, int slot, const double* x_new, int64_t n_new, int d, const double* y_norm,
                          int64_t n_total, int* info);
/* gpbo_lml_batch across the group: the theta search's 1 + n_restarts_optimizer L-BFGS-B runs are independent (sklearn
 * _gpr.py:296-338), so the lanes of a lockstep round are spread over the devices, lane i on device i mod G (n_theta <= 64).
 * X / y_norm non-NULL: made resident on every device first; NULL: the previous call's inputs.  Every lane is bitwise what
 * gpbo_lml returns on any one device, so the search ends at the single-device theta.  lane_device (optional, n_theta):
 * the device each lane ran on. */
int gpbo_group_lml_batch(gpbo_group* grp, int n_theta, const double* X, const double* y_norm, int64_t N, int d, int kernel,
                         const double* length_scales, int n_ls, double noise, int eval_gradient, double* lml, double* grad,
                         int* info, int* lane_device);
/* x_tries (M,d): device r keeps rows [r M / G, (r + 1) M / G) resident (gpbo_group_shard reports the range). */
int gpbo_group_set_candidates(gpbo_group* grp, const double* Xc, int64_t M, int d);
int gpbo_group_shard(const gpbo_group* grp, int rank, int64_t* row_begin, int64_t* row_end);
/* gpbo_generate_candidates_mt19937 across the group: every device generates ITS row block of the reference's candidate
 * matrix from the caller's MT19937 state by jump-ahead — no host sampling, no upload; key / pos come back advanced. */
int gpbo_group_generate_candidates_mt19937(gpbo_group* grp, int64_t M, int d, const double* lo, const double* hi,
                                           uint32_t* key, int* pos);
/* gpbo_posterior on every shard; mu / sd (M,) in global row order, or NULL to keep them on the devices. */
int gpbo_group_posterior(gpbo_group* grp, int slot, double y_mean, double y_std, double* mu, double* sd);
/* gpbo_acq_argbest over all M candidates: global indices, same tie/NaN rules; ys_out (M,) optional. */
int gpbo_group_acq_argbest(gpbo_group* grp, int acq, double acq_param, double y_max, int n_constraints,
                           const double* lb, const double* ub, int k_seeds, int64_t* best_idx, double* best_val,
                           int64_t* seed_idx, double* seed_val, double* ys_out);
int gpbo_group_get_candidate_rows(gpbo_group* grp, const int64_t* idx, int n, double* out);
/* Failure path.  Every gpbo_group_* job has a deadline (GPBO_GROUP_TIMEOUT_S, default 300 s) and every wait for a
 * collective has one (GPBO_COMM_TIMEOUT_S, default 120 s): a device that never comes back, or a peer that never enters
 * the all-gather, turns into GPBO_ERR_COMM (communicators aborted with ncclCommAbort, the group / communicator unusable
 * afterwards) instead of a hung suggest().  A rank whose LOCAL pass failed still enters the all-gather with a poisoned
 * record, so that every rank returns an error from the same step: the failing rank its own code, the others
 * GPBO_ERR_PEER (the exchange completed, the communicators are intact, the group stays usable).  Buffers passed to a
 * gpbo_group_* call that returned GPBO_ERR_COMM because a device missed its deadline must stay allocated until
 * gpbo_group_destroy: a worker released late may still read them (everything the workers WRITE besides the caller's
 * output arrays lives in state owned by the job itself). */

/* ---- calibration (bench.py's roofline: measured peak and sustained clock next to the datasheet numbers) ---- */
/* Sustained v_mfma_f64_16x16x4_f64 rate in TFLOP/s over `iters` dependent-chain-free MFMAs. */
int gpbo_mfma_f64_peak(gpbo_ctx* ctx, int iters, double* tflops);
/* The same MFMA stream with in-kernel clocks, one workgroup of 4 * waves_per_simd (<= 4) waves per compute unit.
 * out[4] = { TFLOP/s over the kernel's own span (first wave's start .. last wave's end, s_memrealtime), shader cycles per
 * MFMA per SIMD, sustained shader clock in MHz (s_memtime / s_memrealtime), event-bracketed kernel milliseconds }.
 * mode 0: accumulators where the compiler puts them (VGPRs); mode 1: AGPR accumulators (inline asm); mode 2: the
 * posterior GEMM's register pattern (2 x 4 tiles, six operand registers). */
int gpbo_mfma_f64_probe(gpbo_ctx* ctx, int iters, int waves_per_simd, int mode, double* out);
/* Streaming copy bandwidth in GB/s (read+write bytes) over a `bytes`-sized buffer. */
int gpbo_hbm_copy_peak(gpbo_ctx* ctx, int64_t bytes, double* gbps);

/* ==== DEBUG BUILD ONLY (-DGPBO_DEBUG: bayesianoptimization_amd/libgpbo_dbg.so) ==========================================
 * Self-test seams, single-kernel timers and micro-benchmarks the tests and scripts/ use.  The product library
 * (libgpbo.so) exports none of them, reads none of the A/B environment switches (GPBO_CHOL_*, GPBO_POST_*, GPBO_SMALL_MAX,
 * GPBO_SELECT_V2*, GPBO_MT_*, GPBO_GEMM128, GPBO_TRI_GRID, GPBO_LML_GRAPH, GPBO_POLISH_FUSED*, GPBO_KG_NS) and contains no scratch-using kernel. */
#ifdef GPBO_DEBUG
/* The optimiser of gpbo_polish_seeds alone, over a host objective (self-test seam: no device, no context): `fg` is called
 * once per lockstep round with the trial points of the runs that are still alive — x (n_live,d) -> f (n_live), g (n_live,d) —
 * and returns 0 or an error code that ends the call.  Same outputs as gpbo_polish_seeds. */
typedef int (*gpbo_fg_callback)(const double* x, int n_live, int d, double* f, double* g, void* user);
int gpbo_debug_minimize_box(gpbo_fg_callback fg, void* user, const double* seeds, int n_seeds, int d, const double* box_lo,
                            const double* box_hi, int max_iter, double* x_out, double* f_out, int* status_out, int* n_rounds_out,
                            int* n_iter_out, int* n_eval_out);

/* The objective of gpbo_polish_seeds' one-launch path (polish_fused.hip; slot 0, no constraints) at each of n <= 64 points (n,d),
 * evaluated `repeat` >= 1 times inside one launch (repeat > 1: for timing an evaluation): out (n, 4 + 3 d) = [f, mu, sd, 0 | df/dx (d) |
 * dmu/dx (d) | dsd/dx (d)] — what gpbo_predict_grad's six kernels compute, from the one kernel (the tests require the same bits). */
int gpbo_debug_polish_eval(gpbo_ctx* ctx, int acq, double acq_param, double y_max, double y_mean, double y_std, const double* points,
                           int n, int d, int repeat, double* out);
/* The objective of gpbo_polish_seeds' lockstep rounds — the path that serves constraint slots — as ONE batched evaluation at n <= 64
 * points (n,d): f_out (n,) and g_out (n,d), the gradient before the optimiser zeroes its non-finite components.  Arguments and
 * refusals as gpbo_polish_seeds (every acquisition kind; GPBO_ACQ_LOG_CEI / GPBO_ACQ_LOG_FEAS with their constraints, which
 * gpbo_debug_polish_eval — no constraint arguments: GPBO_ACQ_LOG_CEI runs there as GPBO_ACQ_LOG_EI, GPBO_ACQ_LOG_FEAS is refused —
 * cannot be given). */
int gpbo_debug_polish_objective(gpbo_ctx* ctx, int acq, double acq_param, double y_max, int n_constraints, const double* lb,
                                const double* ub, const double* y_mean, const double* y_std, const double* points, int n, int d,
                                double* f_out, double* g_out);

/* gpbo_evolve_mixed's objective at each of n points (n, D) in parameter space (transform, posterior of slot 0, -base_acq),
 * evaluated by the kernel of the device walk: out (n,). */
int gpbo_debug_evolve_eval(gpbo_ctx* ctx, int acq, double acq_param, double y_max, double y_mean, double y_std, int n_groups,
                           const int* kind, const int* col0, const int* ncols, const double* points, int n, int D, double* out);
/* gpbo_evolve_mixed's walk over a fixed analytic objective the host can reproduce bit for bit: f(x) = sum_t w_t (g_t - a_t)^2 left
 * to right without contraction, g_t = rint(x_t) on int columns and x_t elsewhere; NaN where x_0 < nan_below, +inf where
 * x_0 > inf_above.  budget = evaluations per launch; launches_out (optional) = launches the run took. */
int gpbo_debug_evolve_walk(gpbo_ctx* ctx, const double* weights, const double* targets, double nan_below, double inf_above,
                           int n_groups, const int* kind, const int* col0, const int* ncols, const double* bounds_lo,
                           const double* bounds_hi, const double* init, int S, int D, int maxiter, int budget, unsigned* key,
                           int* pos, double* x_out, double* f_out, int* nit_out, int* nfev_out, int* success_out,
                           int* launches_out);

/* Multi-GPU failure path, self-test seam (no device needed): a group of workers without contexts, and a job in which
 * rank `fail_rank` returns `fail_code` and rank `hang_rank` sleeps `hang_ms` (either may be -1). */
int gpbo_group_debug_create(int n_ranks, gpbo_group** out);
int gpbo_group_debug_run(gpbo_group* grp, int fail_rank, int fail_code, int hang_rank, int hang_ms);
/* Fault injection: the next gpbo_comm_acq_argbest on `ctx` behaves as if its local pass had failed (it still enters the
 * exchange, with a poisoned record). */
int gpbo_debug_fail_next_acq(gpbo_ctx* ctx);
/* The blocked Cholesky alone on an n x n matrix (n a multiple of 64, lower triangle read; replaces LAPACK dpotrf behind
 * sklearn _gpr.py:349): L_out = the factorised buffer (n x n row-major, lower triangle valid), dinv_out = the inverted
 * 64x64 diagonal blocks [n/64][64][64], stamps_out[16] = shader-clock stamps of the first diagonal workgroup's phases
 * , ms_out = best of `iters` device times, info_out = LAPACK-style pivot info.  variant must be 3 (the 128-column
 * schedule; 2, the round-2 schedule, is retired).  Any output pointer may be NULL. */
int gpbo_debug_cholesky(gpbo_ctx* ctx, const double* A, int64_t n, int variant, int iters, double* L_out, double* dinv_out,
                        long long* stamps_out, double* ms_out, int* info_out);
/* C = alpha * A(m,k) * op(B) + beta * C on the fit GEMM kernel; b_trans: B given as (n,k). */
int gpbo_debug_gemm(gpbo_ctx* ctx, int m, int n, int k, double alpha, const double* A,
                    const double* B, int b_trans, double beta, double* C);
/* The same kernel timed on device-resident random operands: out[2] = { ms per launch, TFLOP/s } (lower_only counts half
 * the flops); a_trans: A given as (k,m). */
int gpbo_debug_gemm_bench(gpbo_ctx* ctx, int m, int n, int k, int b_trans, int a_trans, int lower_only, int iters,
                          double* out);
/* The selection launches of gpbo_acq_argbest alone — ys.argmin(), argsort(ys)[:k] (bayes_opt/acquisition.py:313-317) — over
 * caller-supplied values ys (M,): idx_out / val_out (k,) = the k smallest keys in order (index -1 = fewer than k values),
 * first_nan_out = lowest index holding NaN or -1, ms_out = milliseconds per selection over `iters` repeats.  variant 1: k
 * block-reduction passes (what GPBO_SELECT_V2=0 switches gpbo_acq_argbest back to); variant 2: threshold + rank counting
 * (the default; GPBO_SELECT_V2_CAP bounds its LDS list, beyond which it falls back to the passes).  Same picks, bit for
 * bit.  Overwrites the context's acquisition values. */
int gpbo_debug_select(gpbo_ctx* ctx, const double* ys, int64_t M, int k, int variant, int iters, int64_t* idx_out,
                      double* val_out, int64_t* first_nan_out, float* ms_out);
/* Single-wave instruction latency / issue-cost probe: out[t] = shader cycles for 64 copies of pattern t (latency_probe.hip
 * lists the patterns; t = 0 is the empty bracket).  n <= 32. */
int gpbo_debug_latency_probe(gpbo_ctx* ctx, long long* out, int n);
/* fp64 VALU FMA throughput next to the matrix pipe, 4 waves/SIMD. cfg 0: 16 MFMA per iteration only, 1: 256
 * v_fma_f64 (scalar-operand) only, 2: 16 MFMA + 256 VALU, 3: 16 + 128, 4: 8 + 256.
 * out[3] = { kernel ms, MFMA TFLOP/s, VALU TFLOP/s }. */
int gpbo_hybrid_probe(gpbo_ctx* ctx, int iters, int cfg, double* out);
/* The stages of the int8 posterior pass (posterior_i8.hip) alone, each through the production kernels and launch rule, so that
 * a test can compare them with exact integer arithmetic on the host (tests/i8_reference.py).  S = 7 digit planes; operands in
 * fragment order, [block of 16 items][64-step][plane][lane 16 g + item] 16 bytes.  None of them touches a model slot.
 * gpbo_debug_i8_pack_w: wd_row_scale_kernel + wd_pack_kernel on a host matrix W (NP x NP row-major, NP a multiple of 64, 1 <= N
 * <= NP): Wd_out = the raw digit buffer of the lower triangle (block b of 16 rows holds the steps 0 ... b / 4: (NP / 16 + 2 q (q - 1))
 * S 64 fragments, q = NP / 64), wexp_out / wscale_out (NP,) = the rows' exponents and the epilogue's powers of two. */
int gpbo_debug_i8_pack_w(gpbo_ctx* ctx, const double* W, int64_t N, int64_t NP, void* Wd_out, int* wexp_out, double* wscale_out);
/* The k* generation for the model of slot 0 and the resident candidates [m0, m0 + ldk) (multiples of 64 inside the candidate set
 * padded to 128), by its digit branch and by its fp64 branch.  NP = the model's padded size, by which the caller sized the
 * buffers (GPBO_ERR_INVALID if it is not): Kd_out = the digit slab (ldk NP S bytes), kst_out = the fp64 slab
 * [NP][ldk], mu_part_out [2][ceil(NP / 256)][ldk] = the partial means of the digit branch, then of the fp64 branch. */
int gpbo_debug_i8_kstar_digits(gpbo_ctx* ctx, int64_t NP, int64_t m0, int64_t ldk, void* Kd_out, double* kst_out, double* mu_part_out);
/* posterior_i8_kernel on caller-supplied operands (raw bytes: digits the packers never produce are allowed): Wd as
 * gpbo_debug_i8_pack_w returns it, wscale (NP,), Kd (M NP S bytes), M a multiple of 64; part_out [ceil(NP / 128)][M] = the
 * sums of v^2 per 128-row chunk. */
int gpbo_debug_i8_gemm(gpbo_ctx* ctx, const void* Wd, const double* wscale, const void* Kd, int64_t NP, int64_t M, double* part_out);
/* The envelope of gpbo_kg_argbest alone (the device function its value kernel calls) on R host-given sets of n_lines lines, a / b
 * (R, n_lines) intercepts / slopes, 1 <= n_lines <= GPBO_MAX_KG_POINTS + 1: out[r] = E[max_j (a_j + b_j Z)] - max_j a_j, NaN for a
 * set with a NaN or infinite entry. */
int gpbo_debug_kg_lines(gpbo_ctx* ctx, const double* a, const double* b, int64_t R, int n_lines, double* out);
/* Kernel milliseconds (HIP events) of the three stages of the context's last gpbo_kg_argbest: ms[0] the points (k*, means, solves),
 * ms[1] the candidate x point covariances (with the candidates' scaling), ms[2] the envelopes.  GPBO_KG_NS = 16 | 32 | 64 forces the
 * covariance kernel's columns per pass. */
int gpbo_debug_kg_stage_ms(gpbo_ctx* ctx, float* ms);
/* Kernel milliseconds (HIP events) of the generator kernel of the context's last gpbo_generate_candidates or
 * gpbo_generate_candidates_trust_region call: the launch alone, without the call's argument upload and synchronise. */
int gpbo_debug_generate_ms(gpbo_ctx* ctx, float* ms);
/* Kernel milliseconds (HIP events) of the value kernel of the context's last gpbo_ehvi_argbest or gpmo_cehvi_argbest (include/gpmo.h;
 * with its feasibility epilogue): the tables and the sum over the boxes, without the upload of levels and boxes and without the
 * selection. */
int gpbo_debug_ehvi_ms(gpbo_ctx* ctx, float* ms);
/* Kernel milliseconds (HIP events) of the two stages of the context's last gpbo_qnei_greedy: ms[0] the draws — the candidates'
 * and the pending points' scaling, per group the path weights and the passes over candidates, training and pending points, the
 * baselines —, ms[1] the q greedy steps (score, selection, update; with keys_out their copies too).  The fetch of the results and
 * the synchronise are in neither. */
int gpbo_debug_qnei_stage_ms(gpbo_ctx* ctx, float* ms);
/* The same two stages of the context's last gpbo_cnei_greedy: ms[0] the draws — per group and slot the path weights, the scalings and
 * the passes over candidates and base points, the baselines, with values_out / viol_out / base_values_out their copies too —,
 * ms[1] the q greedy steps. */
int gpbo_debug_cnei_stage_ms(gpbo_ctx* ctx, float* ms);
/* Kernel milliseconds (HIP events) of the three stages of the context's last gpbo_qnhvi_greedy: ms[0] the draws — the scalings, per
 * slot and group the path weights and the passes over candidates and base points —, ms[1] the front build, ms[2] the q greedy steps
 * (score, selection, update; with keys_out their copies too).  The fetch of the results and the synchronise are in none. */
int gpbo_debug_qnehvi_stage_ms(gpbo_ctx* ctx, float* ms);
/* The same three stages of the context's last gpmo_cnhvi_greedy (include/gpmo.h): ms[0] the draws — per group and slot the path
 * weights, the scalings and the passes over candidates and base points, with values_out / viol_out / base_values_out their copies
 * too —, ms[1] the front build, ms[2] the q greedy steps. */
int gpbo_debug_cnhvi_stage_ms(gpbo_ctx* ctx, float* ms);
/* gpbo_qnhvi_greedy's front build and update rule alone, on host-given values: qnehvi_front_kernel on base_values (2, n_draws, n)
 * — objective-major, as base_values_out — against ref (2,), then the update rule n_insert times per draw, in order, with
 * insert_values (2, n_draws, n_insert).  front_size_out (n_draws,), fronts_out (n_draws, GPBO_MAX_QNEHVI_FRONT, 2).  n_draws in
 * [1, 4096], n in [0, GPBO_MAX_QNEHVI_BASE], n_insert in [0, 4096] (a NULL array with a count of 0 is allowed).  A front that outgrows
 * GPBO_MAX_QNEHVI_FRONT is GPBO_ERR_UNSUPPORTED, as in the main call; the context stays usable.  Touches no model slot. */
int gpbo_debug_qnehvi_fronts(gpbo_ctx* ctx, int n_draws, int n, const double* base_values, const double* ref, int n_insert,
                             const double* insert_values, int* front_size_out, double* fronts_out);
#endif /* GPBO_DEBUG */

/* ---- product entry points declared behind the debug block ------------------------------- */
/* Why here: the order-of-calls contract classifies every function declared BEFORE the debug block in one table
 * (tests/test_call_order_cover_host.py); entry points added after that table was closed are declared in this trailing section and
 * classified by its sibling, tests/test_call_order_cover_ext_host.py.  They are product symbols like the ones above: libgpbo.so
 * exports them, and the ABI version does not change (nothing above changed meaning). */

/* Batch noisy expected improvement UNDER CONSTRAINTS, built greedily over the resident candidates from joint posterior draws of the
 * objective and of every constraint (Letham, Karrer, Ottoni & Bakshy 2019, "Constrained Bayesian optimization with noisy
 * experiments", in gpbo_qnei_greedy's greedy, cached-draws form).  gpbo_qnei_greedy with the masked draw g_t in place of f_t.
 * Slots and inputs.  The objective is slot 0, constraint j is slot j, j = 1 .. C, C = n_constraints in [1, GPBO_MAX_MODELS - 1]; the
 * slots' N, kernel kind, length scales, scale and precision may differ.  y_mean / y_std (1 + C,); lb / ub (C,) under
 * gpbo_sample_paths_constrained's rules (no NaN, lb < ub, infinite sides allowed).  T = G S draws, G = n_groups <=
 * GPBO_MAX_QNEI_GROUPS, S = n_paths <= GPBO_MAX_PATHS, F = n_features.  The inputs are concatenated slot-major, then group-major:
 * omega (1 + C, G, F, d), phase (1 + C, G, F), weights (1 + C, G, S, F), eps = slot j's (G, S, N_j) block, one after another.
 * Draws.  Draw t = g S + s of slot j is gpbo_sample_paths' f_s for slot j and group g's inputs, the same bits.  Per draw t and
 * point x:
 *   viol_t(x) = gpbo_sample_paths_constrained's rule: the terms max(max(lb_j - c, c - ub_j), 0) / y_std_j, c = constraint j's draw t
 *               at x, added in constraint order, a NaN kept — the bits that call's viol_out has for group g's inputs
 *   g_t(x)    = NaN if f_t(x) or viol_t(x) is NaN;  f_t(x) if viol_t(x) == 0;  -inf otherwise
 * An infinite raw draw value is outside the contract.
 * Incumbents.  base (n_base, d; host, parameter space): the observed points, then the pending ones; n_base in
 * [0, GPBO_MAX_CNEI_BASE], n_base = 0 with NULL is allowed.  Each slot scales base by its own length scales on the device, as
 * gpbo_qnhvi_greedy does.  m_t = fmax(y_floor, the fmax fold in index order of g_t(base_i)), y_floor finite: a draw in which no
 * observed or pending point is feasible starts from y_floor (Letham et al.'s M); a NaN is dropped by the fold.  baseline_out (T,) =
 * m_t before the first pick.  There is no `noisy` flag: plain constrained Monte-Carlo qEI is base = the pending points and y_floor =
 * the best feasible measurement.
 * Steps, picks, updates: gpbo_qnei_greedy's exactly, with g_t in place of f_t — the same term, the same order of adds, ONE division,
 * the mask to +inf, the selection's rules (the first NaN wins, else the least key, ties to the lowest index).  -inf needs no special
 * case: -inf - m_t is not > 0, so the term is 0, and fmax(m_t, -inf) = m_t — an infeasible pick leaves every incumbent as it is.
 * When no draw finds a feasible candidate above its incumbent every gain is exactly 0 and the zero-gain tail applies (the lowest
 * unpicked index); there is no least-violation fallback.  pick_feasible[j] = (the number of t with g_t(pick) > -inf) / T: the
 * share of draws that call the pick feasible, NaN for a NaN pick.
 * Outputs.  pick_idx, pick_gain, pick_feasible (q,) and baseline_out (T,).  Optional (NULL: not fetched): values_out (1 + C, T, M),
 * the RAW per-slot draws; viol_out (T, M); base_values_out (1 + C, T, n_base), raw; keys_out (q, M), every step's keys (a debugging
 * aid: one copy per step).
 * On the device: per group, in slot order 1 .. C then 0, per slot one launch_path_weights, the candidates and the base points scaled
 * by THAT slot's length scales, and one pass of path_eval_kernel over each.  The constraint passes fold into one per-group
 * viol[S][M] and one viol[S][n_base]; the objective's pass reads them and writes rows [g S, (g + 1) S) of the (T, M) block and of
 * base[T][n_base] through the PATH_MASKED epilogue.  No (1 + C, T, M) block exists: values_out is staged one (slot, group) at a
 * time.  Then gpbo_qnei_greedy's own stream — qnei_baseline_kernel (y_best = y_floor over the whole row), qnei_score_kernel, the
 * selection — and cnei_update_kernel, which files {gain, index, feasible}.  Everything crosses behind ONE synchronisation.  fp64
 * whatever a slot's precision.  Workspace: the context's own — the block 8 T M bytes, one group's violations 8 S M (+ 8 S M for the
 * stage with values_out), at the base points 8 (T + S) n_base (+ 8 S n_base with base_values_out), the base points as given and
 * scaled 8 n_base (d + DP) (DP = d padded to the kernels' width), the incumbents 16 T, the records 24 q and the mask M bytes —;
 * grown on demand and kept; an allocation that fails is GPBO_ERR_HIP.
 * A reader, as gpbo_sample_paths: the fits, the resident mu / sd, what gpbo_posterior_refresh may still refresh, the candidates and
 * the negative-variance flag stay as they were; the context's acquisition values are overwritten.
 * GPBO_ERR_INVALID: n_constraints outside [1, GPBO_MAX_MODELS - 1]; n_groups outside [1, GPBO_MAX_QNEI_GROUPS]; n_paths outside
 * [1, GPBO_MAX_PATHS] or n_features outside [1, GPBO_MAX_PATH_FEATURES]; a NULL y_mean / y_std / lb / ub / omega / phase / weights /
 * eps / pick_idx / pick_gain / pick_feasible / baseline_out; a y_std not finite or not positive, a y_mean not finite; a NaN bound
 * or lb >= ub; y_floor not finite; n_base outside [0, GPBO_MAX_CNEI_BASE], n_base > 0 with a NULL or non-finite base; d not the
 * slots'; q outside [1, GPBO_MAX_SEEDS], q > M.  GPBO_ERR_STATE: one of the slots 0 .. C unfitted or with a fit pending, no resident
 * candidates, candidates of another d.  There is no gpbo_group_* / gpbo_comm_* form. */
#define GPBO_MAX_CNEI_BASE 16384      /* observed + pending points */
int gpbo_cnei_greedy(gpbo_ctx* ctx, int n_constraints, const double* y_mean, const double* y_std,
                     const double* lb, const double* ub,
                     int n_groups, int n_paths, int n_features,
                     const double* omega, const double* phase, const double* weights, const double* eps,
                     double y_floor, const double* base, int n_base, int d,
                     int q, int64_t index_offset,
                     int64_t* pick_idx, double* pick_gain, double* pick_feasible, double* baseline_out,
                     double* values_out, double* viol_out, double* base_values_out, double* keys_out);

#ifdef __cplusplus
}
#endif
#endif /* GPBO_H */
