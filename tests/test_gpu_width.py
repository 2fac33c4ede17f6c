"""GPU (-m gpu): every device path at every padded-width tier, up to GPBO_MAX_DIM = 64 columns, against the oracle.

Every kernel pads the input width to DP = pad_dim(d) in {4, 8, 16, 32, 64} and has its own instantiation or branch per tier; the
widest tier carries the largest LDS images, the most registers and the wave reductions over rows 2 and 3 (d > 32).  The widths
below sit on both sides of every tier boundary (4|5, 8|9, 16|17, 32|33) plus a partly filled and a full 64 tier, and the
problems are built so that every column matters (`problem`):

  * inputs uniform on [0, 1]^d with length scales that grow with sqrt(d): at d = 64 with d-independent length scales K is close
    to the identity and k* close to 0 — the posterior would be the prior whatever a kernel does with column 50;
  * a DIFFERENT length scale per column (geometric, 0.6x .. 1.6x), so a column permutation or a length-scale/column mismatch
    changes the answer;
  * a target built from every column (sin(X w), w nonzero everywhere), so alpha and mu depend on all of them;
  * the single-live-column probe (`probe`): at d = 64 every column constant but column t, so K depends on column t alone — a
    kernel that loses, duplicates or mis-strides that column sees a matrix of ones (plus noise) instead.

tests/test_width_discrimination_host.py applies those plausible bugs to the oracle and shows each moves the compared quantities
by more than 100x the bars below, so these tests can fail.  Bars: those the existing tests hold for the same quantity (K 1e-14,
L 1e-10, W and alpha 1e-8, LML 1e-10, its gradient 1e-7 of the largest component, the posterior 1e-9 Matern / 1e-8 RBF, fp32 1e-7
on mu and 2e-5 y_std^2 on the variance); kappa(K) of each case is part of every assert message."""
import numpy as np
import pytest

from bayesianoptimization_amd.engine import F32
from conftest import elementwise_err, rel_err
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

WIDTHS = (4, 5, 8, 9, 16, 17, 32, 33, 48, 63, 64)
SLOW_WIDTHS = (5, 17, 33, 64)
PROBE_COLS = (0, 15, 16, 31, 32, 47, 48, 63)
KERNELS = (O.MATERN25, O.RBF)
NOISE = 1e-6
KNAME = {O.MATERN25: "matern", O.RBF: "rbf"}


def length_scale(d, kernel, per_dim=True):
    """0.5 sqrt(d) (Matern) / 0.45 sqrt(d) (RBF) times a geometric 0.6 .. 1.6 spread over the columns.  Below 8 columns (RBF:
    below 16) the scale is shorter: a thousand points in 4 .. 9 dimensions at the longer one put kappa(K + 1e-6 I) at 1e8 and
    beyond (RBF's spectrum decays fastest), where two correct CPU algorithms already differ by the bars below."""
    if kernel == O.MATERN25:
        f = 0.5 if d >= 8 else 0.35
    else:
        f = 0.45 if d >= 16 else (0.2 if d >= 8 else 0.12)
    s = f * np.sqrt(d)
    return s * np.geomspace(0.6, 1.6, d) if per_dim else np.array([s])


def target(X, rng):
    d = X.shape[1]
    w = rng.uniform(0.5, 1.5, d) * np.where(np.arange(d) % 2, -1.0, 1.0) * 4.0 / np.sqrt(d)
    return np.sin(X @ w) + 0.05 * rng.standard_normal(X.shape[0])


def problem(N, d, kernel, per_dim=True, M=0, seed=0):
    """(X, y, ls, Xc): N observations and M candidates (one of them ON training point 3) in [0, 1]^d, every column live."""
    rng = np.random.RandomState(seed * 100003 + 97 * N + d + 7 * kernel)
    X = rng.uniform(size=(N, d))
    y = target(X, rng)
    Xc = rng.uniform(size=(M, d))
    if M:
        Xc[min(7, M - 1)] = X[3]
    return X, y, length_scale(d, kernel, per_dim), Xc


def probe(N, t, kernel, M=0, d=64, seed=0):
    """Single live column t: every other column is a (per-column different) constant; column t holds a jittered grid 0.8 of its
    own length scale apart, in random order (uniform points on a line would put kappa(K) at the noise floor).  K, k*, mu, sd
    depend on column t alone and d LML / d log(l_s) is exactly 0 for s != t."""
    rng = np.random.RandomState(seed * 1009 + 13 * t + N + kernel)
    ls = length_scale(d, kernel, True)
    const = rng.uniform(size=d)
    step = 0.8 * ls[t]
    X = np.tile(const, (N, 1))
    X[:, t] = (rng.permutation(N) + rng.uniform(-0.25, 0.25, N)) * step
    y = np.sin(2.0 * X[:, t] / ls[t]) + 0.05 * rng.standard_normal(N)
    Xc = np.tile(const, (M, 1))
    Xc[:, t] = rng.uniform(-1.0, N, size=M) * step
    if M:
        Xc[min(7, M - 1)] = X[3]
    return X, y, ls, Xc


#: worst error / bar and kappa(K) per path at d = 64, written as JSON to the file GPBO_WIDTH_REPORT names (if set) at the end
WORST = {}


def record(path, ratio, kap):
    if ratio >= WORST.get(path, (-1.0, 0.0))[0]:
        WORST[path] = (float(ratio), float(kap))


@pytest.fixture(scope="module", autouse=True)
def _width_report():
    yield
    import json
    import os

    out = os.environ.get("GPBO_WIDTH_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump({k: {"worst_err_over_bar": r, "kappa": c} for k, (r, c) in sorted(WORST.items())}, f, indent=1)


def kernel_with_noise(kernel, X, ls):
    K = O.kernel_matrix(kernel, X, None, ls)
    K[np.diag_indices_from(K)] += NOISE
    return K


def kappa(kernel, X, ls):
    ev = np.linalg.eigvalsh(kernel_with_noise(kernel, X, ls))
    return float(ev[-1] / ev[0])


def lml_oracle(kernel, X, yn, ls):
    """O.log_marginal_likelihood with the (N, N, d) tensor of squared differences walked in row blocks (at N = 2048, d = 64 it
    would be 2 GB): the same formula, sklearn _gpr.py:575-652."""
    ls = np.atleast_1d(np.asarray(ls, dtype=np.float64))
    lml = O.log_marginal_likelihood(kernel, X, yn, ls, NOISE, eval_gradient=False)
    L = np.linalg.cholesky(kernel_with_noise(kernel, X, ls))
    from scipy.linalg import cho_solve
    alpha = cho_solve((L, True), yn)
    inner = np.outer(alpha, alpha) - cho_solve((L, True), np.eye(X.shape[0]))
    Xs = X / ls
    grad = np.zeros(ls.shape[0])
    for a in range(0, X.shape[0], 128):
        D = (Xs[a:a + 128, None, :] - Xs[None, :, :]) ** 2
        d2 = D.sum(-1)
        if kernel == O.MATERN25:
            tmp = np.sqrt(5 * d2)
            g = 5.0 / 3.0 * (tmp + 1) * np.exp(-tmp)
        else:
            g = np.exp(-0.5 * d2)
        w = inner[a:a + 128] * g
        grad += 0.5 * (np.array([np.sum(w * d2)]) if ls.shape[0] == 1 else np.einsum("ij,ijt->t", w, D))
    return lml, grad


def post_tol(kernel):
    return 1e-8 if kernel == O.RBF else 1e-9


def check_posterior(mu, sd, gp, Xc, kernel, what):
    mu_o, sd_o = O.predict(gp, Xc)
    tol = post_tol(kernel)
    e_mu, e_sd = rel_err(mu, mu_o), rel_err(sd, sd_o)
    assert e_mu <= tol and e_sd <= tol, f"{what}: mu {e_mu:.2e}, sd {e_sd:.2e} (bar {tol:.0e})"
    e_sd1, e_mu1 = elementwise_err(sd, sd_o, mu, mu_o, gp.y_std)
    assert e_sd1 <= 1e-5 and e_mu1 <= 1e-5, f"{what}: per candidate sd {e_sd1:.2e}, mu {e_mu1:.2e}"
    return max(e_mu, e_sd) / tol


def check_fit(engine, X, yn, kernel, ls, what, slot=0):
    """K, L, W, alpha, triu(L) == 0 and L L^T against K (test_fit_parity's bars).  Returns the worst error / bar."""
    N = X.shape[0]
    gp = O.fit_fixed_theta(kernel, X, yn, ls, NOISE, normalize_y=False)
    K = kernel_with_noise(kernel, X, ls)
    Lg = engine.get_L(N, slot)
    errs = {"K": (rel_err(engine.get_K(N, slot), K), 1e-14), "L": (rel_err(Lg, gp.L), 1e-10),
            "W": (rel_err(engine.get_Linv(N, slot), np.linalg.inv(gp.L)), 1e-8),
            "alpha": (rel_err(engine.get_alpha(N, slot), gp.alpha), 1e-8), "LLt": (rel_err(Lg @ Lg.T, K), 1e-13)}
    msg = f"{what}: " + ", ".join(f"{k} {e:.2e}" for k, (e, _) in errs.items())
    for k, (e, bar) in errs.items():
        assert e < bar, f"{k} over its bar {bar:.0e} -- {msg}"
    assert np.all(np.triu(Lg, 1) == 0.0), msg
    return max(e / bar for e, bar in errs.values())


FIT_NS = (50, 300, 1000)     # NP = 64: the one-workgroup kernel; NP = 320: the strip path; NP = 1024: the multi-launch sequence
FIT_CASES = [(N, d, k, pd) for N in FIT_NS for d in WIDTHS for k in KERNELS for pd in (True, False)]


@pytest.mark.parametrize("N,d,kernel,per_dim", FIT_CASES,
                         ids=[f"N{N}-d{d}-{KNAME[k]}-{'ard' if pd else 'iso'}" for N, d, k, pd in FIT_CASES])
def test_fit_at_every_width(engine, N, d, kernel, per_dim):
    X, y, ls, _ = problem(N, d, kernel, per_dim)
    yn, _, _ = O.normalize_targets(y)
    engine.fit(X, yn, kernel, ls, NOISE)
    kap = kappa(kernel, X, ls)
    r = check_fit(engine, X, yn, kernel, ls, f"N={N} d={d} kappa={kap:.1e}")
    if d == 64:
        record(f"fit N={N}", r, kap)


@pytest.mark.parametrize("N", (50, 300, 1000))
@pytest.mark.parametrize("kernel", KERNELS, ids=["matern", "rbf"])
@pytest.mark.parametrize("t", PROBE_COLS)
def test_single_live_column_fit_and_posterior(engine, t, kernel, N):
    """K from column t alone (a kernel that loses it sees ones + noise), the posterior over candidates that differ in column t
    only, at d = 64 on each fit path."""
    X, y, ls, Xc = probe(N, t, kernel, M=1001)
    yn, ym, ys = O.normalize_targets(y)
    engine.fit(X, yn, kernel, ls, NOISE)
    kap = kappa(kernel, X, ls)
    what = f"probe t={t} N={N} kappa={kap:.1e}"
    record(f"probe fit N={N}", check_fit(engine, X, yn, kernel, ls, what), kap)
    mu, sd = engine.predict(Xc, y_mean=ym, y_std=ys)
    record(f"probe posterior N={N}", check_posterior(mu, sd, O.fit_fixed_theta(kernel, X, y, ls, NOISE), Xc, kernel, what), kap)


# -- LML + gradient -----------------------------------------------------------------------------------------------------
LML_CASES = [(N, d, k) for N in FIT_NS for d in WIDTHS for k in KERNELS]


def check_lml(lml, grad, lml_o, grad_o, what):
    e_v = abs(lml - lml_o) / max(1.0, abs(lml_o))
    e_g = np.max(np.abs(grad - grad_o)) / max(np.max(np.abs(grad_o)), 1e-12)
    assert e_v <= 1e-10 and e_g <= 1e-7, f"{what}: value {e_v:.2e}, gradient {e_g:.2e} (argmax {int(np.argmax(np.abs(grad - grad_o)))})"
    return max(e_v / 1e-10, e_g / 1e-7)


@pytest.mark.parametrize("N,d,kernel", LML_CASES, ids=[f"N{N}-d{d}-{KNAME[k]}" for N, d, k in LML_CASES])
def test_lml_and_gradient_at_every_width(engine, N, d, kernel):
    """gpbo_lml with per-dimension length scales (a d-component gradient) and with a scalar one, against the oracle; the lanes
    of gpbo_lml_batch bitwise gpbo_lml."""
    X, y, ls, _ = problem(N, d, kernel, seed=1)
    yn, _, _ = O.normalize_targets(y)
    kap = kappa(kernel, X, ls)
    what = f"N={N} d={d} kappa={kap:.1e}"
    lml, grad = engine.lml(X, yn, kernel, ls, NOISE)
    assert grad.shape == (d,)
    r = check_lml(lml, grad, *lml_oracle(kernel, X, yn, ls), what)
    if d == 64:
        record(f"lml N={N}", r, kap)
    iso = ls[:1] * 1.1
    lml1, grad1 = engine.lml(X, yn, kernel, iso, NOISE)
    check_lml(lml1, grad1, *lml_oracle(kernel, X, yn, iso), what + " iso")
    lanes = np.vstack([ls, ls * 0.8, ls[::-1]])
    for (v, g), row in zip(engine.lml_batch(X, yn, kernel, lanes, NOISE), lanes):
        v1, g1 = (lml, grad) if row is lanes[0] else engine.lml(X, yn, kernel, row, NOISE)
        assert v == v1 and np.array_equal(g, g1), what


@pytest.mark.parametrize("N", (50, 300, 1000))
@pytest.mark.parametrize("kernel", KERNELS, ids=["matern", "rbf"])
@pytest.mark.parametrize("t", PROBE_COLS)
def test_single_live_column_lml_gradient(engine, t, kernel, N):
    """Component t carries the whole gradient, the other 63 are 0 to rounding — in gpbo_lml and in a gpbo_lml_batch lane."""
    X, y, ls, _ = probe(N, t, kernel)
    yn, _, _ = O.normalize_targets(y)
    kap = kappa(kernel, X, ls)
    what = f"probe t={t} N={N} kappa={kap:.1e}"
    lml, grad = engine.lml(X, yn, kernel, ls, NOISE)
    lml_o, grad_o = lml_oracle(kernel, X, yn, ls)
    assert np.count_nonzero(grad_o) == 1 and grad_o[t] != 0.0
    record(f"probe lml N={N}", check_lml(lml, grad, lml_o, grad_o, what), kap)
    others = np.delete(grad, t)
    assert np.max(np.abs(others)) <= 1e-12 * abs(grad[t]), what
    (v, g), = engine.lml_batch(X, yn, kernel, ls[None, :], NOISE)
    assert v == lml and np.array_equal(g, grad), what


@pytest.mark.parametrize("kernel", KERNELS, ids=["matern", "rbf"])
def test_lml_per_lane_stream_path_at_64_columns(engine, kernel):
    """N = 2048 (NP >= 2048: the lanes of gpbo_lml_batch on their own streams) with 64 per-dimension length scales."""
    X, y, ls, _ = problem(2048, 64, kernel, seed=2)
    yn, _, _ = O.normalize_targets(y)
    kap = kappa(kernel, X, ls)
    what = f"N=2048 d=64 kappa={kap:.1e}"
    lml, grad = engine.lml(X, yn, kernel, ls, NOISE)
    record("lml N=2048", check_lml(lml, grad, *lml_oracle(kernel, X, yn, ls), what), kap)
    (v0, g0), (v1, g1) = engine.lml_batch(X, yn, kernel, np.vstack([ls, 0.9 * ls]), NOISE)
    assert v0 == lml and np.array_equal(g0, grad), what
    v1s, g1s = engine.lml(X, yn, kernel, 0.9 * ls, NOISE)
    assert v1 == v1s and np.array_equal(g1, g1s), what


# -- posterior paths ----------------------------------------------------------------------------------------------------
# (N, M): M <= 8 the batched-GEMV path; NP <= 256 the 8-wave fused kernel with both ends in the launch; 384 <= NP <= 512 with
# 9216 <= Mp <= 16384 the 16-wave fused kernel (v4); NP > 512 the k* slab + GEMM pipeline (v3).  Ragged candidate counts.
POST_PATHS = {"small": (300, 5), "fused8": (200, 4099), "v4": (450, 16001), "slab": (1000, 20001)}
POST_CASES = [(p, d, k) for p in POST_PATHS for d in WIDTHS for k in KERNELS]


@pytest.mark.parametrize("path,d,kernel", POST_CASES, ids=[f"{p}-d{d}-{KNAME[k]}" for p, d, k in POST_CASES])
def test_posterior_paths_at_every_width(engine, path, d, kernel):
    N, M = POST_PATHS[path]
    X, y, ls, Xc = problem(N, d, kernel, per_dim=d % 2 == 1 or d == 64, M=M, seed=3)
    yn, ym, ys = O.normalize_targets(y)
    engine.fit(X, yn, kernel, ls, NOISE)
    engine.set_candidates(Xc)
    mu, sd = engine.posterior(0, ym, ys)
    kap = kappa(kernel, X, ls)
    r = check_posterior(mu, sd, O.fit_fixed_theta(kernel, X, y, ls, NOISE), Xc, kernel, f"{path} N={N} M={M} d={d} kappa={kap:.1e}")
    if d == 64:
        record(f"posterior {path}", r, kap)


@pytest.mark.parametrize("N", (300, 1000))
@pytest.mark.parametrize("d", SLOW_WIDTHS)
def test_f32_posterior_at_every_width(engine, d, N):
    """fp32 mode (test_gpu_f32's bars): mu 1e-7, |sd^2 - sd_ref^2| <= 2e-5 y_std^2; the factorisation stays fp64."""
    kernel = O.MATERN25 if d in (5, 33) else O.RBF
    X, y, ls, Xc = problem(N, d, kernel, M=5003, seed=4)
    yn, ym, ys = O.normalize_targets(y)
    gp = O.fit_fixed_theta(kernel, X, y, ls, NOISE)
    engine.fit(X, yn, kernel, ls, NOISE, precision=F32)
    kap = kappa(kernel, X, ls)
    what = f"f32 N={N} d={d} kappa={kap:.1e}"
    assert rel_err(engine.get_L(N), gp.L) < 1e-10, what
    engine.set_candidates(Xc)
    mu, sd = engine.posterior(0, ym, ys)
    mu_o, sd_o = O.predict(gp, Xc)
    assert rel_err(mu, mu_o) < 1e-7, what
    assert np.max(np.abs(sd ** 2 - sd_o ** 2)) < 2e-5 * ys ** 2, what
    if d == 64:
        record(f"posterior f32 N={N}", max(rel_err(mu, mu_o) / 1e-7, np.max(np.abs(sd ** 2 - sd_o ** 2)) / (2e-5 * ys ** 2)), kap)


# -- predict_grad / predict_cov / fit_append -----------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS, ids=["matern", "rbf"])
@pytest.mark.parametrize("d", (33, 64))
def test_predict_grad_and_cov_at_wide_widths(engine, d, kernel):
    """test_predict_grad_equals_the_oracle_gradient's and test_predict_cov_equals_sklearn_return_cov's bars."""
    X, y, ls, Xq = problem(300, d, kernel, M=64, seed=5)
    yn, ym, ys = O.normalize_targets(y)
    gp = O.fit_fixed_theta(kernel, X, y, ls, NOISE)
    engine.fit(X, yn, kernel, ls, NOISE)
    kap = kappa(kernel, X, ls)
    what = f"d={d} kappa={kap:.1e}"
    mu, sd, dmu, dsd = engine.predict_grad(Xq, 0, ym, ys)
    mu_o, sd_o, dmu_o, dsd_o = O.predict_grad(gp, Xq)
    assert rel_err(mu, mu_o) < 1e-8 and rel_err(sd, sd_o) < 1e-7, what
    assert rel_err(dmu, dmu_o) < 1e-7 and rel_err(dsd, dsd_o) < 1e-6, (what, rel_err(dmu, dmu_o), rel_err(dsd, dsd_o))
    if d == 64:
        record("predict_grad", max(rel_err(mu, mu_o) / 1e-8, rel_err(sd, sd_o) / 1e-7, rel_err(dmu, dmu_o) / 1e-7,
                                   rel_err(dsd, dsd_o) / 1e-6), kap)
    mu, cov = engine.predict_cov(Xq[:40], 0, ym, ys)
    mu_o, cov_o = O.predict_cov(gp, Xq[:40])
    assert rel_err(mu, mu_o) < 1e-8, what
    assert np.max(np.abs(cov - cov_o)) < 1e-8 * np.max(np.abs(cov_o)), what
    if d == 64:
        record("predict_cov", max(rel_err(mu, mu_o) / 1e-8, np.max(np.abs(cov - cov_o)) / (1e-8 * np.max(np.abs(cov_o)))), kap)


@pytest.mark.parametrize("kernel", KERNELS, ids=["matern", "rbf"])
@pytest.mark.parametrize("d", (33, 64))
def test_fit_append_at_wide_widths(engine, d, kernel):
    """100 rows, then 20 at once, then one: each time the model of a from-scratch fit (test_fit_append_equals_full_fit's bars)."""
    X, y, ls, Xc = problem(121, d, kernel, M=300, seed=6)
    tol = 1e-9 if kernel == O.MATERN25 else 1e-6
    n = 100
    yn, _, _ = O.normalize_targets(y[:n])
    engine.fit(X[:n], yn, kernel, ls, NOISE)
    for k in (20, 1):
        n += k
        yn, ym, ys = O.normalize_targets(y[:n])
        engine.fit_append(X[n - k:n], yn)
        kap = kappa(kernel, X[:n], ls)
        what = f"n={n} d={d} kappa={kap:.1e}"
        gp = O.fit_fixed_theta(kernel, X[:n], yn, ls, NOISE, normalize_y=False)
        assert rel_err(engine.get_K(n), kernel_with_noise(kernel, X[:n], ls)) < 1e-14, what
        assert rel_err(engine.get_L(n), gp.L) < tol, what
        assert rel_err(engine.get_Linv(n) @ gp.L, np.eye(n)) < 100 * tol, what
        assert rel_err(engine.get_alpha(n), gp.alpha) < 100 * tol, what
        mu, sd = engine.predict(Xc, y_mean=ym, y_std=ys)
        mu_o, sd_o = O.predict(gp, Xc)
        assert rel_err(mu, ys * mu_o + ym) < tol and rel_err(sd, ys * sd_o) < tol, what
        if d == 64:
            record(f"fit_append +{k}", max(rel_err(engine.get_L(n), gp.L) / tol, rel_err(mu, ys * mu_o + ym) / tol,
                                           rel_err(sd, ys * sd_o) / tol, rel_err(engine.get_alpha(n), gp.alpha) / (100 * tol)), kap)


# -- fused local search -------------------------------------------------------------------------------------------------
@pytest.fixture
def polish_any_size():
    import os

    old = os.environ.get("GPBO_POLISH_FUSED_MAX_NP")
    os.environ["GPBO_POLISH_FUSED_MAX_NP"] = "512"
    yield
    if old is None:
        os.environ.pop("GPBO_POLISH_FUSED_MAX_NP", None)
    else:
        os.environ["GPBO_POLISH_FUSED_MAX_NP"] = old


POLISH_CASES = [(N, d) for d in (33, 48, 64) for N in (64, 128, 192, 384, 512)]


@pytest.mark.parametrize("N,d", POLISH_CASES)
def test_one_fused_local_search_evaluation_at_wide_widths(debug_engine, polish_any_size, N, d):
    """test_gpu_polish_fused's single-evaluation comparison on both sides of plan_polish's LDS decisions (csrc/search_plan.h) (W in LDS at NP = 64
    / 128 if its image fits, W in memory from 192 on; X staged or not)."""
    from test_gpu_polish_fused import _polish_eval

    eng = debug_engine
    kernel = O.MATERN25 if (N // 64 + d) % 2 else O.RBF
    X, y, ls, _ = problem(N, d, kernel, seed=7)
    yn, ym, ys = O.normalize_targets(y)
    eng.fit(X, yn, kernel, ls, NOISE, slot=0)
    rng = np.random.RandomState(5)
    pts = np.vstack([rng.uniform(size=(7, d)), X[:2] + 1e-6, np.full((1, d), 0.5)])
    kappa_ucb = 2.576
    got = _polish_eval(eng, O.UCB, kappa_ucb, 0.0, ym, ys, pts)
    mu, sd, dmu, dsd = eng.predict_grad(pts, slot=0, y_mean=ym, y_std=ys)
    kap = kappa(kernel, X, ls)
    what = f"N={N} d={d} kappa={kap:.1e}"
    eps = np.finfo(np.float64).eps
    Kst = O.kernel_matrix(kernel, pts, X, ls)
    alpha, Wm = eng.get_alpha(N), eng.get_Linv(N)
    term_mu = ys * (np.abs(Kst) @ np.abs(alpha))
    assert np.all(np.abs(got["mu"] - mu) <= 512 * eps * term_mu + 1e-15), what
    V, absV = Kst @ Wm.T, np.abs(Kst) @ np.abs(Wm).T
    term_var = ys * ys * 2.0 * np.sum(np.abs(V) * absV, axis=1)
    assert np.all(np.abs(got["sd"] ** 2 - sd ** 2) <= 512 * eps * term_var + 1e-15 * ys * ys), what
    amp_mu = max(1.0, float(np.max(term_mu)) / max(float(np.abs(mu).max()), ys))
    amp_w = max(1.0, float(np.max(term_var)) / (ys * ys))
    assert np.max(np.abs(got["dmu"] - dmu)) <= 2e-13 * amp_mu * float(np.abs(dmu).max()), what
    far = sd > 1e-3 * ys
    if far.any():
        assert np.max(np.abs(got["dsd"][far] - dsd[far])) <= 1e-11 * amp_w * amp_w * float(np.abs(dsd[far]).max()), what
    assert np.max(np.abs(got["f"] + (got["mu"] + kappa_ucb * got["sd"]))) <= 1e-15 * max(float(np.abs(mu).max()), ys), what
    assert np.allclose(got["g"], -(got["dmu"] + kappa_ucb * got["dsd"]), rtol=1e-14, atol=0), what
    gp = O.fit_fixed_theta(kernel, X, y, ls, NOISE)
    mu_o, sd_o = O.predict(gp, pts)
    assert np.allclose(got["mu"], mu_o, rtol=0, atol=1e-7 * max(1.0, float(np.abs(mu_o).max()))), what
    assert np.allclose(got["sd"], sd_o, rtol=0, atol=1e-6 * float(sd_o.max())), what
    _, _, dmu_o, dsd_o = O.predict_grad(gp, pts)
    assert rel_err(got["dmu"], dmu_o) < 1e-7, what
    if d == 64:
        record(f"local search N={N}", max(np.max(np.abs(got["mu"] - mu_o)) / (1e-7 * max(1.0, float(np.abs(mu_o).max()))),
                                          np.max(np.abs(got["sd"] - sd_o)) / (1e-6 * float(sd_o.max())),
                                          rel_err(got["dmu"], dmu_o) / 1e-7), kap)


# -- the whole random stage at 64 columns ---------------------------------------------------------------------------------
def _all_rows(engine, M, d):
    return np.vstack([engine.get_candidate_rows(np.arange(a, min(M, a + 4096)), d) for a in range(0, M, 4096)])


def test_random_stage_at_64_columns(engine):
    """N = 512, M = 65 536 candidates drawn on the device from the caller's MT19937 stream, posterior, EI, arg-best: the oracle's
    candidates, values, arg-best index and top 16 exactly."""
    N, d, M, K_SEEDS = 512, 64, 65536, 16
    kernel = O.MATERN25
    X, y, ls, _ = problem(N, d, kernel, seed=8)
    yn, ym, ys = O.normalize_targets(y)
    gp = O.fit_fixed_theta(kernel, X, y, ls, NOISE)
    engine.fit(X, yn, kernel, ls, NOISE)
    lo, hi = np.zeros(d), np.ones(d)
    ref, dev = np.random.RandomState(17), np.random.RandomState(17)
    want = np.column_stack([ref.uniform(lo[t], hi[t], M) for t in range(d)])
    engine.generate_candidates_like(M, lo, hi, dev)
    assert dev.uniform() == ref.uniform()
    Xc = _all_rows(engine, M, d)
    assert np.array_equal(Xc, want)
    mu, sd = engine.posterior(0, ym, ys)
    mu_o, sd_o = np.empty(M), np.empty(M)
    for a in range(0, M, 8192):
        mu_o[a:a + 8192], sd_o[a:a + 8192] = O.predict(gp, Xc[a:a + 8192])
    kap = kappa(kernel, X, ls)
    what = f"kappa={kap:.1e}"
    assert rel_err(mu, mu_o) <= 1e-9 and rel_err(sd, sd_o) <= 1e-9, (what, rel_err(mu, mu_o), rel_err(sd, sd_o))
    assert max(elementwise_err(sd, sd_o, mu, mu_o, ys)) <= 1e-5, what
    y_max = float(y.max())
    ys_o = -1 * O.base_acq(O.EI, mu_o, sd_o, 0.01, y_max)
    bi, bv, si, sv, yv = engine.acq_argbest(O.EI, 0.01, y_max, k_seeds=K_SEEDS, return_values=True)
    order = np.argsort(ys_o, kind="stable")
    assert rel_err(yv, ys_o) <= 1e-8, what
    assert bi == int(order[0]) and bv == yv[bi], what
    assert np.array_equal(si, order[:K_SEEDS]), (what, si, order[:K_SEEDS])
    record("random stage N=512 M=65536", max(rel_err(mu, mu_o) / 1e-9, rel_err(sd, sd_o) / 1e-9, rel_err(yv, ys_o) / 1e-8), kap)


def test_mixed_space_with_a_one_hot_width_of_64(engine):
    """Float + int + categorical parameters whose kernel-space width is exactly 64 (14 + 1 + 16 + 16 + 17 columns): candidates
    assembled and kernel-transformed on the device, the posterior over them == the one over space.kernel_transform(rows)
    uploaded from the host, bit for bit, and the oracle's."""
    from sklearn.gaussian_process.kernels import Matern

    from bayesianoptimization_amd import fused_acquisition as A
    from bayesianoptimization_amd.float_space import MixedSpace
    from bayesianoptimization_amd.gpr import HipGPR

    pb = {f"f{i:02d}": (0.0, 1.0 + 0.1 * i) for i in range(14)}
    pb["n"] = (-3, 7, int)
    pb["c1"] = tuple(f"a{i}" for i in range(16))
    pb["c2"] = tuple(f"b{i}" for i in range(16))
    pb["c3"] = tuple(f"c{i}" for i in range(17))
    sp = MixedSpace(pb)
    M = 20001
    rng = np.random.RandomState(4)
    Xobs = sp.random_sample(300, rng)
    Z = sp.kernel_transform(Xobs)
    assert Z.shape[1] == 64
    y = target(Z, rng)
    ls = length_scale(64, O.MATERN25, True)
    gp = HipGPR(kernel=Matern(nu=2.5, length_scale=ls), alpha=NOISE, normalize_y=True, optimizer=None, engine=engine,
                transform=sp.kernel_transform).fit(Xobs, y)
    groups = A._mixed_groups_on_device([gp], sp, np.random.RandomState(0), M)
    assert groups is not None
    ref, dev = np.random.RandomState(77), np.random.RandomState(77)
    want = sp.random_sample(M, ref)
    engine.generate_candidates_mixed(M, groups, dev)
    assert np.array_equal(_all_rows(engine, M, sp.dim), want)
    engine.transform_candidates(groups)
    gp._ensure_resident()
    ym, ys = float(gp._y_train_mean), float(gp._y_train_std)
    mu_d, sd_d = engine.posterior(0, ym, ys)
    Zc = sp.kernel_transform(want)
    mu_h, sd_h = engine.predict(Zc, y_mean=ym, y_std=ys)
    assert np.array_equal(mu_d, mu_h) and np.array_equal(sd_d, sd_h)
    kap = kappa(O.MATERN25, Z, ls)
    record("mixed space (one-hot 64)", check_posterior(mu_d, sd_d, O.fit_fixed_theta(O.MATERN25, Z, y, ls, NOISE), Zc, O.MATERN25,
                                                       f"mixed kappa={kap:.1e}"), kap)


# -- the 64 | 65 edge -----------------------------------------------------------------------------------------------------
def test_65_columns_are_refused_and_leave_the_context_usable(engine):
    """gpbo_lml, gpbo_lml_batch, gpbo_set_candidates and gpbo_generate_candidates at d = 65 raise the mapped exception; a d = 64
    fit on the same context then gives the bits it gives on a fresh context."""
    from bayesianoptimization_amd.engine import GpEngine

    X65, y65, _, _ = problem(40, 65, O.MATERN25)
    yn65, _, _ = O.normalize_targets(y65)
    with pytest.raises((NotImplementedError, ValueError)):
        engine.lml(X65, yn65, O.MATERN25, 1.0, NOISE)
    with pytest.raises((NotImplementedError, ValueError)):
        engine.lml_batch(X65, yn65, O.MATERN25, np.array([[1.0], [2.0]]), NOISE)
    with pytest.raises((NotImplementedError, ValueError)):
        engine.set_candidates(np.zeros((10, 65)))
    with pytest.raises((NotImplementedError, ValueError)):
        engine.generate_candidates(1000, np.zeros(65), np.ones(65), 3)
    X, y, ls, Xc = problem(300, 64, O.MATERN25, M=2001, seed=9)
    yn, ym, ys = O.normalize_targets(y)
    out = []
    with GpEngine(0) as fresh:
        for eng in (engine, fresh):
            eng.fit(X, yn, O.MATERN25, ls, NOISE)
            eng.set_candidates(Xc)
            out.append((eng.get_L(300), eng.get_alpha(300)) + tuple(eng.posterior(0, ym, ys)))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_hipgpr_default_settings_at_65_and_64_columns(engine):
    """A default HipGPR (lml_on_device="auto"): at 65 columns one warning and scikit-learn's fit and predict, bit for bit; at 64
    columns the device path, whose theta search over 64 per-dimension length scales reaches scikit-learn's optimum to the LML bar."""
    import warnings

    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import Matern

    from bayesianoptimization_amd.gpr import HipGPR

    X, y, _, Xq = problem(60, 65, O.MATERN25, M=20, seed=10)
    k = Matern(nu=2.5, length_scale=np.full(65, 3.0))
    sk = GaussianProcessRegressor(kernel=k, alpha=NOISE, normalize_y=True, random_state=1).fit(X, y)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        gp = HipGPR(kernel=k, alpha=NOISE, normalize_y=True, random_state=1, engine=engine).fit(X, y)
    said = [w for w in seen if issubclass(w.category, UserWarning) and "HIP path" in str(w.message)]
    assert len(said) == 1, [str(w.message) for w in seen]
    assert gp._host_mode
    assert np.array_equal(gp.kernel_.theta, sk.kernel_.theta)
    assert np.array_equal(gp.L_, sk.L_) and np.array_equal(gp.alpha_, sk.alpha_)
    for a, b in zip(gp.predict(Xq, return_std=True), sk.predict(Xq, return_std=True)):
        assert np.array_equal(a, b)

    X, y, ls, _ = problem(100, 64, O.MATERN25, seed=11)
    k = Matern(nu=2.5, length_scale=ls, length_scale_bounds=(1e-2, 1e3))
    sk = GaussianProcessRegressor(kernel=k, alpha=NOISE, normalize_y=True, random_state=2).fit(X, y)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        gp = HipGPR(kernel=k, alpha=NOISE, normalize_y=True, random_state=2, engine=engine).fit(X, y)
    assert not [w for w in seen if "HIP path" in str(w.message)]
    assert not gp._host_mode and gp.kernel_.theta.shape == (64,)
    # the two searches may step differently: their optima agree in LML value, each evaluated by scikit-learn
    lml_sk = sk.log_marginal_likelihood_value_
    lml_gp = GaussianProcessRegressor.log_marginal_likelihood(sk, gp.kernel_.theta)
    assert abs(lml_gp - lml_sk) <= 1e-10 * max(1.0, abs(lml_sk)), (lml_gp, lml_sk)
    assert abs(gp.log_marginal_likelihood_value_ - lml_sk) <= 1e-10 * max(1.0, abs(lml_sk))
