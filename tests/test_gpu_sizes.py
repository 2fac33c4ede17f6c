"""GPU (-m gpu): every training-set size tier of the product library on both sides of its boundary, against the oracle.

The device code switches path, tiling or schedule at values of NP = round_up(N, 64) (csrc/gpbo_api.hip, posterior_kernel.hip,
posterior_small.hip).  The N and M lists below put a case on both sides of each switch of the PRODUCT rule (no GPBO_* variable
is set here; tests/test_size_discrimination_host.py checks the lists against a restatement of the rules):

  * fit path: one workgroup if NP <= 64, the strip path if NP <= 768, the multi-launch sequence above (`last_timings()` shows which
    ran: the per-phase events exist on the multi-launch path only);
  * trtri's ragged pairs, whose second block has b2 < b rows: b2 = 64 ... 1984 (NP = 832: 64, 320; 896: 128, 384; 960 and 3008:
    64, 192, 448 (960); 4032: up to 1984; none at NP = 2048 and 4096);
  * the Cholesky's outer panel: NP (<= 2048), 1024 (<= 4096), 512 beyond with a ragged last panel; the look-ahead from NP = 4096 on;
    an odd count of 64-row blocks (NP = 4032, 4160, 5056);
  * the LML gradient: K^-1 tile by tile up to NP = 768, W^T W above; lml_batch lane groups at NP >= 2048 and >= 4096, and the
    hipGraph a shape is replayed from after its second call — on NEW data of that shape too;
  * the posterior: GEMV up to small_batch_limit(NP), then path 2 / 3 / 4 by row chunks and Mp, the fused ends, the pinned output
    copy up to M = 4096 — every candidate against the oracle, and the arg-best / top 16 of UCB and EI;
  * gpbo_fit_append's row append, rebuild, growth and rebuild inside grown capacity; a slot reused at a smaller NP and DP.

Bars: the suite's own for each quantity — K 1e-14, L 1e-10, W L - I and alpha 1e-7 (test_fit_append_equals_full_fit's 100 x 1e-9),
the LML 1e-10 relative and its gradient 1e-7 of its largest component, fp64 mu / sd 1e-9 and the acquisition 1e-8 with the arg-best
and top 16 exact (test_gpu_large_path.py), fp32 mu 1e-7 and |sd^2 - sd_ref^2| <= 2e-5 y_std^2 (test_gpu_f32.py).  The length scale
f sqrt(d) takes f from a table per (kernel, d, N tier) so that kappa(K + 1e-6 I) stays in [1e3, 5e6] — every case asserts it:
below, K is close to I and a lost block of W hardly shows; above, two correct CPU algorithms already differ by these bars."""
import numpy as np
import pytest
from scipy.linalg import cho_solve, cholesky

from bayesianoptimization_amd.engine import F32
from conftest import elementwise_err, rel_err
from helpers import assert_same_model
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

NOISE = 1e-6
KAPPA_WINDOW = (1e3, 5e6)
KNAME = {O.MATERN25: "matern", O.RBF: "rbf"}
TIERS = (128, 600, 1100, 2200, 1 << 16)          # upper N of each length-scale tier
#: f per (kernel, d, per-dimension) and N tier; measured kappa(K + 1e-6 I) on uniform [0, 1]^d inputs is in the notebook (§12)
LS_FACTOR = {
    (O.MATERN25, 5, False): (0.4, 0.24, 0.16, 0.12, 0.12),
    (O.RBF, 5, True): (0.3, 0.14, 0.1, 0.08, 0.08),
    (O.MATERN25, 17, True): (0.7, 0.45, 0.3, 0.25, 0.2),
    (O.RBF, 17, False): (0.5, 0.3, 0.2, 0.2, 0.2),
}
SHAPES = tuple(LS_FACTOR)


def length_scale(kernel, d, per_dim, N):
    f = LS_FACTOR[(kernel, d, per_dim)][next(i for i, n in enumerate(TIERS) if N <= n)]
    s = f * np.sqrt(d)
    return s * np.geomspace(0.75, 1.33, d) if per_dim else np.array([s])


def make_data(N, d, seed, M=0):
    """N inputs uniform on [0, 1]^d, a target from every column, and M candidates (number 7 ON training point 3)."""
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(N, d))
    w = rng.uniform(0.5, 1.5, d) * np.where(np.arange(d) % 2, -1.0, 1.0) * 4.0 / np.sqrt(d)
    y = np.sin(X @ w) + 0.05 * rng.standard_normal(N)
    Xc = rng.uniform(size=(M, d))
    if M:
        Xc[min(7, M - 1)] = X[3]
    return X, y, Xc


def kernel_with_noise(kernel, X, ls):
    K = O.kernel_matrix(kernel, X, None, ls)
    K[np.diag_indices_from(K)] += NOISE
    return K


def kappa(K, L, iters=60):
    """kappa(K) from the Rayleigh quotients of power iteration (lambda_max; kernel matrices have a large first gap) and of inverse
    iteration through the Cholesky factor (lambda_min): a lower bound that is within a few per cent of eigvalsh's at these sizes,
    at O(N^2) per step instead of an O(N^3) eigensolver."""
    v = np.ones(K.shape[0])
    for _ in range(iters):
        v = K @ v
        v /= np.linalg.norm(v)
    u = np.random.RandomState(0).standard_normal(K.shape[0])
    for _ in range(iters):
        u = cho_solve((L, True), u)
        u /= np.linalg.norm(u)
    return float((v @ K @ v) * (u @ cho_solve((L, True), u)))


def check_kappa(kap, what):
    assert KAPPA_WINDOW[0] <= kap <= KAPPA_WINDOW[1], f"{what}: kappa {kap:.2e} outside {KAPPA_WINDOW} (pick another f)"


def lml_ref(kernel, X, yn, ls, L=None):
    """sklearn's LML and d LML / d log(length_scale) (_gpr.py:575-652; O.log_marginal_likelihood's formula), the (N, N, d) tensor of
    squared differences walked in row blocks."""
    ls = np.atleast_1d(np.asarray(ls, dtype=np.float64))
    N = X.shape[0]
    if L is None:
        L = cholesky(kernel_with_noise(kernel, X, ls), lower=True)
    alpha = cho_solve((L, True), yn)
    lml = -0.5 * float(yn @ alpha) - np.log(np.diag(L)).sum() - N / 2 * np.log(2 * np.pi)
    inner = np.outer(alpha, alpha) - cho_solve((L, True), np.eye(N))
    Xs = X / ls
    grad = np.zeros(ls.shape[0])
    for a in range(0, N, 256):
        D = (Xs[a:a + 256, None, :] - Xs[None, :, :]) ** 2
        d2 = D.sum(-1)
        if kernel == O.MATERN25:
            tmp = np.sqrt(5 * d2)
            g = 5.0 / 3.0 * (tmp + 1) * np.exp(-tmp)
        else:
            g = np.exp(-0.5 * d2)
        w = inner[a:a + 256] * g
        grad += 0.5 * (np.array([np.sum(w * d2)]) if ls.shape[0] == 1 else np.einsum("ij,ijt->t", w, D))
    return lml, grad


def check_lml(lml, grad, lml_o, grad_o, what):
    e_v = abs(lml - lml_o) / max(1.0, abs(lml_o))
    e_g = np.max(np.abs(grad - grad_o)) / max(np.max(np.abs(grad_o)), 1e-12)
    assert e_v <= 1e-10 and e_g <= 1e-7, f"{what}: value {e_v:.2e}, gradient {e_g:.2e}"
    return max(e_v / 1e-10, e_g / 1e-7)


def check_posterior(mu, sd, mu_o, sd_o, ys, what, tol=1e-9):
    e_mu, e_sd = rel_err(mu, mu_o), rel_err(sd, sd_o)
    assert e_mu <= tol and e_sd <= tol, f"{what}: mu {e_mu:.2e}, sd {e_sd:.2e} (bar {tol:.0e})"
    e_sd1, e_mu1 = elementwise_err(sd, sd_o, mu, mu_o, ys)
    assert e_sd1 <= 1e-5 and e_mu1 <= 1e-5, f"{what}: per candidate sd {e_sd1:.2e}, mu {e_mu1:.2e}"
    return max(e_mu, e_sd) / tol


#: worst error / bar and kappa per path, written as JSON to the file GPBO_SIZE_REPORT names (if set) at the end of the module
WORST = {}


def record(path, ratio, kap):
    if ratio >= WORST.get(path, (-1.0, 0.0))[0]:
        WORST[path] = (float(ratio), float(kap))


@pytest.fixture(scope="module", autouse=True)
def _size_report():
    yield
    import json
    import os

    out = os.environ.get("GPBO_SIZE_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump({k: {"worst_err_over_bar": r, "kappa": c} for k, (r, c) in sorted(WORST.items())}, f, indent=1)


class Problem:
    """One (N, kernel, d, length-scale kind): inputs, 300 candidates and the oracle's K, L, W = L^-1, alpha, kappa, mu / sd."""

    def __init__(self, N, kernel, d, per_dim, M=300, seed=0):
        self.N, self.kernel, self.d, self.per_dim = N, kernel, d, per_dim
        self.X, self.y, self.Xc = make_data(N, d, seed * 7919 + 31 * N + d + kernel, M)
        self.yn, self.ym, self.ys = O.normalize_targets(self.y)
        self.ls = length_scale(kernel, d, per_dim, N)
        self.K = kernel_with_noise(kernel, self.X, self.ls)
        self.L = cholesky(self.K, lower=True)
        self.alpha = cho_solve((self.L, True), self.yn)
        self.kappa = kappa(self.K, self.L)
        self.what = f"N={N} {KNAME[kernel]} d={d} {'ard' if per_dim else 'iso'} kappa={self.kappa:.1e}"
        self._lml = None

    @property
    def NP(self):
        return (self.N + 63) // 64 * 64

    def gp(self):
        return O.GPState(self.kernel, np.atleast_1d(self.ls), NOISE, self.X, self.L, self.alpha, self.ym, self.ys)

    def posterior(self, Xc):
        return O.predict(self.gp(), Xc)

    def lml(self):
        if self._lml is None:
            self._lml = lml_ref(self.kernel, self.X, self.yn, self.ls, self.L)
        return self._lml


# -- a / b: fit, posterior, LML at both sides of every tier ---------------------------------------------------------------
FIT_NS = (64, 65, 768, 769, 832, 833, 960, 1088, 1984, 1985, 2049, 2113, 3008, 4032, 4033, 4097, 5003)
FIT_CASES = [(N,) + s for N in FIT_NS for s in SHAPES]


@pytest.fixture(scope="module", params=FIT_CASES,
                ids=[f"N{N}-{KNAME[k]}-d{d}-{'ard' if pd else 'iso'}" for N, k, d, pd in FIT_CASES])
def sized(request):
    """Module scope: pytest runs every test of one problem before it builds the next, so each oracle is computed once."""
    return Problem(*request.param)


def test_fit_at_every_size_tier(engine, sized):
    p = sized
    check_kappa(p.kappa, p.what)
    engine.set_timing(True)
    engine.fit(p.X, p.yn, p.kernel, p.ls, NOISE)
    t = engine.last_timings()
    phases = [t["kmat"], t["cholesky"], t["trtri"]]
    if p.NP <= 768:          # the one-workgroup kernel / the strip path: one fit event, no per-phase ones
        assert t["fit"] > 0 and all(v < 0 for v in phases), (p.what, t)
    else:                    # the multi-launch sequence
        assert t["fit"] > 0 and all(v > 0 for v in phases), (p.what, t)
    N = p.N
    Lg = engine.get_L(N)
    errs = {"K": (rel_err(engine.get_K(N), p.K), 1e-14), "L": (rel_err(Lg, p.L), 1e-10),
            "WL-I": (rel_err(engine.get_Linv(N) @ p.L, np.eye(N)), 1e-7), "alpha": (rel_err(engine.get_alpha(N), p.alpha), 1e-7)}
    msg = f"{p.what}: " + ", ".join(f"{k} {e:.2e}" for k, (e, _) in errs.items())
    for k, (e, bar) in errs.items():
        assert e < bar, f"{k} over its bar {bar:.0e} -- {msg}"
    assert np.all(np.triu(Lg, 1) == 0.0), msg
    path = "fused" if p.NP <= 64 else ("strip" if p.NP <= 768 else "multi-launch")
    record(f"fit {path} N={N}", max(e / bar for e, bar in errs.values()), p.kappa)
    engine.set_candidates(p.Xc)
    mu, sd = engine.posterior(0, p.ym, p.ys)
    mu_o, sd_o = p.posterior(p.Xc)
    record(f"posterior after fit N={N}", check_posterior(mu, sd, mu_o, sd_o, p.ys, p.what + " posterior"), p.kappa)
    assert abs(sd[7] - sd_o[7]) <= 1e-9 * float(sd_o.max()), p.what    # the candidate on a training point


def test_lml_and_gradient_at_every_size_tier(engine, sized):
    p = sized
    lml, grad = engine.lml(p.X, p.yn, p.kernel, p.ls, NOISE)
    assert grad.shape == (p.ls.shape[0],)
    grad_path = "kinv tiles" if p.NP <= 768 else "WtW"
    record(f"lml ({grad_path}) N={p.N}", check_lml(lml, grad, *p.lml(), p.what), p.kappa)


LANE_NS = (1984, 1985, 4032, 4033)
LANE_FACTORS = (1.0, 0.95, 1.1, 0.97, 1.05, 1.08)


@pytest.mark.parametrize("N", LANE_NS)
def test_lml_batch_lanes_at_the_grouping_tiers(engine, N):
    """Six lanes — one group at NP = 1984, two groups of three at 2048 and 4032, three groups of two at 4096 — each against the
    oracle and bitwise gpbo_lml; per-dimension length scales, one lane with them reversed."""
    p = Problem(N, O.RBF, 5, True, M=0, seed=1)
    lanes = np.vstack([p.ls * f for f in LANE_FACTORS[:5]] + [p.ls[::-1] * LANE_FACTORS[5]])
    got = engine.lml_batch(p.X, p.yn, p.kernel, lanes, NOISE)
    assert len(got) == len(lanes)
    for i, ((v, g), row) in enumerate(zip(got, lanes)):
        K = kernel_with_noise(p.kernel, p.X, row)
        L = cholesky(K, lower=True)
        kap = kappa(K, L)
        what = f"lane {i} N={N} kappa={kap:.1e}"
        check_kappa(kap, what)
        record(f"lml_batch N={N}", check_lml(v, g, *lml_ref(p.kernel, p.X, p.yn, row, L), what), kap)
        v1, g1 = engine.lml(p.X, p.yn, p.kernel, row, NOISE)
        assert v == v1 and np.array_equal(g, g1), what


# -- c: the lml_batch graph, replayed on new data of the same shape --------------------------------------------------------
@pytest.mark.parametrize("N", (1088, 2113))
def test_lml_batch_graph_replay_on_new_data(engine, N):
    """Same (N, d, kernel, n_ls, noise) five times: new X and y (the first call launches directly, the second captures and replays),
    new y only, new X only, reuse_inputs=True; then a different lane count.  Every lane matches the oracle of THAT call's data and
    is bitwise gpbo_lml on it — a graph that kept the previous problem's inputs would not."""
    kernel, d = O.MATERN25, 5
    ls0 = length_scale(kernel, d, False, N)
    X0, y0, _ = make_data(N, d, 100 + N)
    X1, y1, _ = make_data(N, d, 200 + N)
    X3, y2, _ = make_data(N, d, 300 + N)
    y2 = O.normalize_targets(y2)[0]
    calls = [(X0, O.normalize_targets(y0)[0], False, 4), (X1, O.normalize_targets(y1)[0], False, 4), (X1, y2, False, 4),
             (X3, y2, False, 4), (X3, y2, True, 4), (X0, y2, False, 3)]
    oracle = {}
    for c, (X, yn, reuse, n_lanes) in enumerate(calls):
        lanes = ls0[None, :] * np.array(LANE_FACTORS[:n_lanes])[:, None]
        got = engine.lml_batch(X, yn, kernel, lanes, NOISE, reuse_inputs=reuse)
        for i, ((v, g), row) in enumerate(zip(got, lanes)):
            key = (id(X), id(yn), float(row[0]))
            if key not in oracle:
                K = kernel_with_noise(kernel, X, row)
                L = cholesky(K, lower=True)
                kap = kappa(K, L)
                check_kappa(kap, f"call {c} lane {i}")
                oracle[key] = lml_ref(kernel, X, yn, row, L) + (kap,)
            lml_o, grad_o, kap = oracle[key]
            what = f"call {c} lane {i} N={N} kappa={kap:.1e}"
            record(f"lml_batch replay N={N}", check_lml(v, g, lml_o, grad_o, what), kap)
            v1, g1 = engine.lml(X, yn, kernel, row, NOISE)
            assert v == v1 and np.array_equal(g, g1), what


# -- d: the posterior dispatch grid of the product rule -------------------------------------------------------------------
def small_batch_limit(NP):
    """posterior_small.hip's rule (product build)."""
    return 48 if NP <= 512 else 512 if NP <= 1024 else 256 if NP <= 2048 else 128 if NP <= 4096 else 72


MP_EDGES = (8064, 8065, 9088, 9089, 16384, 16385, 32640, 32641)     # Mp = 8064 | 8192, 9088 | 9216, 16384 | 16512, 32640 | 32768
POST_NPS = (256, 320, 448, 512, 576, 832, 1088, 2112, 4160)


def post_ms(NP):
    """The candidate counts whose dispatch differs on the two sides: the GEMV limit, the pinned output copy (M <= 4096) and, with
    two row chunks (256 < NP <= 512), the Mp edges of paths 2 / 3 / 4."""
    lim = small_batch_limit(NP)
    ms = {lim, lim + 1, 4096, 4097}
    if 256 < NP <= 512:
        ms.update(MP_EDGES)
    return sorted(ms)


POST_CASES = [(NP, M) for NP in POST_NPS for M in post_ms(NP)]


def _post_shape(NP):
    return SHAPES[POST_NPS.index(NP) % len(SHAPES)]


@pytest.fixture(scope="module")
def post_problem(request):
    """N = NP - 7 (ragged padding), candidates for the largest M of this NP and the oracle on all of them."""
    NP = request.param
    kernel, d, per_dim = _post_shape(NP)
    p = Problem(NP - 7, kernel, d, per_dim, M=max(post_ms(NP)), seed=2)
    p.mu_o, p.sd_o = np.empty(p.Xc.shape[0]), np.empty(p.Xc.shape[0])
    for a in range(0, p.Xc.shape[0], 4096):
        p.mu_o[a:a + 4096], p.sd_o[a:a + 4096] = p.posterior(p.Xc[a:a + 4096])
    return p


@pytest.mark.parametrize("post_problem,M", POST_CASES, indirect=["post_problem"], ids=[f"NP{n}-M{m}" for n, m in POST_CASES])
def test_posterior_dispatch_of_the_product_rule(engine, post_problem, M):
    p = post_problem
    check_kappa(p.kappa, p.what)
    engine.fit(p.X, p.yn, p.kernel, p.ls, NOISE)
    Xc, mu_o, sd_o = p.Xc[:M], p.mu_o[:M], p.sd_o[:M]
    engine.set_candidates(Xc)
    mu, sd = engine.posterior(0, p.ym, p.ys)
    what = f"{p.what} M={M}"
    r = check_posterior(mu, sd, mu_o, sd_o, p.ys, what)
    y_max = float(p.y.max())
    for acq, param in ((O.UCB, 2.576), (O.EI, 0.01)):
        ys_o = -1 * O.base_acq(acq, mu_o, sd_o, param, y_max)
        bi, bv, si, sv, ys = engine.acq_argbest(acq, param, y_max, k_seeds=16, return_values=True)
        order = np.argsort(ys_o, kind="stable")
        e = rel_err(ys, ys_o)
        assert e <= 1e-8, f"{what} acq {acq}: {e:.2e}"
        assert bi == int(order[0]) and bv == ys[bi], what
        assert np.array_equal(si, order[:16]), (what, si, order[:16])
        r = max(r, e / 1e-8)
    record(f"posterior NP={p.NP}", r, p.kappa)


F32_CASES = [(NP, M) for NP in (448, 512) for M in MP_EDGES]


@pytest.mark.parametrize("post_problem,M", F32_CASES, indirect=["post_problem"], ids=[f"NP{n}-M{m}" for n, m in F32_CASES])
def test_f32_posterior_at_the_mp_edges(engine, post_problem, M):
    """fp32 mode (test_gpu_f32's bars: mu 1e-7, |sd^2 - sd_ref^2| <= 2e-5 y_std^2); the factorisation stays fp64."""
    p = post_problem
    engine.fit(p.X, p.yn, p.kernel, p.ls, NOISE, precision=F32)
    assert rel_err(engine.get_L(p.N), p.L) < 1e-10, p.what
    engine.set_candidates(p.Xc[:M])
    mu, sd = engine.posterior(0, p.ym, p.ys)
    mu_o, sd_o = p.mu_o[:M], p.sd_o[:M]
    e_mu, e_var = rel_err(mu, mu_o), float(np.max(np.abs(sd ** 2 - sd_o ** 2))) / p.ys ** 2
    assert e_mu < 1e-7 and e_var < 2e-5, f"{p.what} M={M}: mu {e_mu:.2e}, var {e_var:.2e}"
    record(f"posterior f32 NP={p.NP}", max(e_mu / 1e-7, e_var / 2e-5), p.kappa)


# -- e: fit_append across the tiers ---------------------------------------------------------------------------------------
def _append_run(eng, shape, n0, steps, seed):
    """Fit n0 rows, then append `steps` rows per call; after every call the model of a from-scratch fit (assert_same_model, at its
    bars: 1e-9 Matern, 1e-6 RBF).  The length scale is the one of the final N's tier."""
    kernel, d, per_dim = shape
    X, y, Xc = make_data(n0 + sum(steps), d, seed, M=300)
    ls = length_scale(kernel, d, per_dim, X.shape[0])
    tol = 1e-9 if kernel == O.MATERN25 else 1e-6
    n = n0
    eng.fit(X[:n], O.normalize_targets(y[:n])[0], kernel, ls, NOISE)
    for k in steps:
        n += k
        yn, ym, ys = O.normalize_targets(y[:n])
        eng.fit_append(X[n - k:n], yn)
        K = kernel_with_noise(kernel, X[:n], ls)
        kap = kappa(K, cholesky(K, lower=True))
        check_kappa(kap, f"n={n}")
        r = assert_same_model(eng, X[:n], yn, kernel, ls, NOISE, ym, ys, Xc, tol=tol)
        record(f"fit_append {n0}->{X.shape[0]} {KNAME[kernel]}", r, kap)
    return n


@pytest.mark.parametrize("shape", (SHAPES[0], SHAPES[3]), ids=["matern-d5", "rbf-d17"])
def test_fit_append_across_the_strip_boundary(engine, shape):
    """760 -> 770 one row at a time: row appends at NP = 768 (strip path), the rebuild into NP = 832 (multi-launch), a row append
    there."""
    assert _append_run(engine, shape, 760, [1] * 10, seed=41) == 770


def test_fit_append_row_appends_then_a_rebuild_at_the_same_np(engine):
    """1000 -> 1005 by single rows (the row-append kernel at NP = 1024), then 17 rows at once: N = 1022, NP still 1024, n_new > 16
    rebuilds."""
    assert _append_run(engine, SHAPES[2], 1000, [1] * 5 + [17], seed=42) == 1022


def test_fit_append_growth_and_a_rebuild_inside_grown_capacity():
    """A fresh context: fit 2000 rows (capacity NP = 2048), append to 2100 (NP = 2112: the slot grows by 25 %, Xs copied), append to
    2240 (NP = 2240 < cap_NP: a rebuild with leading dimension NP inside the larger buffers, outer panel 1024)."""
    from bayesianoptimization_amd.engine import GpEngine

    with GpEngine(0) as eng:
        assert _append_run(eng, SHAPES[1], 2000, [100, 140], seed=43) == 2240


# -- f: a slot reused at smaller sizes ------------------------------------------------------------------------------------
def _model_state(eng, p, Ms):
    N = p.N
    out = {"K": eng.get_K(N), "L": eng.get_L(N), "W": eng.get_Linv(N), "alpha": eng.get_alpha(N)}
    for M in Ms:
        eng.set_candidates(p.Xc[:M])
        out[f"mu{M}"], out[f"sd{M}"] = eng.posterior(0, p.ym, p.ys)
    return out


def test_slot_reuse_at_smaller_sizes_is_bitwise_a_fresh_fit(engine):
    """N = 4161, d = 17 in slot 0; then N = 833, 100, 40 (d = 17) and 40 (d = 5) in the same slot, whose buffers stay at the first
    fit's size: each bitwise a fresh context's fit of the same data — K, L, W, alpha and mu / sd below and above the GEMV limit —
    and within the oracle's bars."""
    from bayesianoptimization_amd.engine import GpEngine

    big = Problem(4161, O.MATERN25, 17, True, M=0, seed=3)
    engine.fit(big.X, big.yn, big.kernel, big.ls, NOISE)
    assert rel_err(engine.get_L(big.N), big.L) < 1e-10
    for N, d in ((833, 17), (100, 17), (40, 17), (40, 5)):
        kernel = O.MATERN25
        p = Problem(N, kernel, d, d == 17, M=700, seed=4)
        lim = small_batch_limit(p.NP)
        Ms = (lim, min(lim + 150, 700))
        engine.fit(p.X, p.yn, kernel, p.ls, NOISE)
        reused = _model_state(engine, p, Ms)
        with GpEngine(0) as fresh:
            fresh.fit(p.X, p.yn, kernel, p.ls, NOISE)
            want = _model_state(fresh, p, Ms)
        for k in want:
            assert np.array_equal(reused[k], want[k]), f"{p.what}: {k} differs from a fresh context's"
        if p.N >= 100:
            check_kappa(p.kappa, p.what)
        assert rel_err(reused["K"], p.K) < 1e-14 and rel_err(reused["L"], p.L) < 1e-10, p.what
        assert rel_err(reused["W"] @ p.L, np.eye(N)) < 1e-7 and rel_err(reused["alpha"], p.alpha) < 1e-7, p.what
        mu_o, sd_o = p.posterior(p.Xc[:Ms[1]])
        r = check_posterior(reused[f"mu{Ms[1]}"], reused[f"sd{Ms[1]}"], mu_o, sd_o, p.ys, p.what)
        r = max(r, check_posterior(reused[f"mu{Ms[0]}"], reused[f"sd{Ms[0]}"], mu_o[:Ms[0]], sd_o[:Ms[0]], p.ys, p.what))
        record(f"slot reuse N={N} d={d}", r, p.kappa)
