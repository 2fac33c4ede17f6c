"""GPU (-m gpu): the order-of-calls contract of a long-lived context.  Every kernel is compared with the oracle in isolation by the
other modules; each of those tests builds its state from scratch.  A maximize() loop keeps one context alive for hundreds of steps,
and in that time the library trusts state it derived once: per slot the int8 digit planes of W (Wd / wscale / wd_valid), W^T in the
K buffer (wt_valid), the fp32 packing (Wp32), wp_packed, M_post, fitted and buffers larger than the current NP; per context the
resident candidates, the resident theta-search inputs, the graph pool of gpbo_lml_batch and the negative-variance flag.

Call fit, fit_begin / fit_wait, fit_append, lml(slot) and set_candidates / generate_candidates* / transform_candidates the WRITERS and
every other call a READER.  Pinned here:

  1. readers are invisible: after writers with readers in between, a call returns bit for bit what it returns on a fresh context
     that ran the same writers alone;
  2. a full fit erases the past, whatever the slot held: another size, another precision, a failed fit, cached Wd / W^T / Wp32;
  3. gpbo_lml_batch touches no slot;
  4. a slot that a writer left unfitted raises the STATE error on every reader.

`replay` runs a list of steps on the shared engine (on top of whatever earlier tests left there); `replay_fresh` opens, for every
checked step, a fresh context, runs the writers that precede the step (and the reads the step names in `needs`) and then the step
itself — one context per checked step, so that the fresh side never carries a cache a reader made.  Equality is bitwise
(test_bitwise_determinism, the graph-replay tests and test_the_product_library_runs_the_same_search establish that these paths are
run-to-run deterministic).  Two runs could be wrong in the same way, so every scenario also holds its final state to the oracle at
the bar of the test that covers that quantity in isolation: check_posterior / check_lml of test_gpu_sizes.py, assert_same_model
(tests/helpers.py: 1e-9 for Matern) for a model reached by appends, test_gpu_f32.py's bars in F32 mode, the 1e-14 of K,
the 1e-8 / exact arg-best of the acquisition, _same_or_better of test_gpu_polish_fused.py for a search.  No tolerance is new.

Routes: the int8 GEMM (PostPath::SlabI8) is established as test_gpu_int8_posterior.py does — the debug build's default pass is
bitwise its GPBO_POST_KERNEL=8 pass (and not its =3 pass); N = 300 is NP = 320 > SEARCH_LDS_NP = 128: SearchMode::WInMemory
(search_plan.h; tests/test_search_plan_host.py pins the rule), N = 100 is NP = 128: WInLds; N = 800 is NP = 832 > 768:
FitTier::Blocked, the graph-eligible tier (fit_plan.h).

The sampling, batch and Pareto entry points (gpbo_sample_paths, gpbo_sample_paths_constrained, gpbo_ascend_paths, gpbo_mes_argbest,
gpbo_kg_argbest, gpbo_ehvi_argbest, gpbo_qnei_greedy, gpbo_qnhvi_greedy, gpbo_generate_candidates_trust_region) are held to the same
contract, against each other, by tests/test_gpu_call_order_sampling.py, which imports Step, W, R, replay and replay_fresh from here.
The per-context state they share with each other and with gpbo_acq_argbest:
  ctx->ys            [M] acquisition values for acq_argbest, mes, kg, ehvi and for the qnei / qnehvi keys; [S][M] negated path values
                     for sample_paths; launch_values_argbest selects over the values ALREADY in it;
  ctx->Xcs           re-scaled with ONE slot's length scales by posterior, posterior_refresh, kg, sample_paths, qnei and qnehvi
                     (qnehvi leaves slot 1's scaling behind);
  ctx->red           the selection's SelState | picks | partial | nan_partial, AND the trust-region generator's Sobol tables, the
                     MT19937 key, the mixed-space flags and the fit scalars; enqueue_select and the generators call `ensure`, which
                     frees and reallocates when a later call needs more; qnei_update_kernel and qnehvi_update_kernel take SelState*
                     and Key* pointers into it at launch time;
  pinned_aux + PIN_AUX_SEL_OUT   fetch_selection, launch_topk_rows and the qnei / qnehvi pick records cross in this one window;
  the six workspaces ctx->paths, cpaths, kg, ehvi, qnei, qnehvi: each grown by `ensure` (free, then malloc), laid out by T, M, B, d, q;
  func_attrs         ATTR_KG and ATTR_EHVI are per-context, first-use settings;
  the per-slot posterior   M_post, refreshable, M_refresh, N_post, ystd_post: between fit_append and posterior_refresh it is stale
                     but refreshable, which is where a batch loop sits between two picks.

SCENARIOS lists, per scenario of this file, the library functions it runs as readers; tests/test_call_order_cover_host.py holds the
two files' lists against include/gpbo.h, so that a new entry point cannot stay outside the contract."""
import os

import numpy as np
import pytest
from scipy.linalg import cho_solve, cholesky

from bayesianoptimization_amd import _lib
from bayesianoptimization_amd.engine import F32, F64, GpEngine
from conftest import rel_err
from helpers import assert_same_model
from oracle import gp_oracle as O
from test_gpu_polish_fused import _same_or_better
from test_gpu_sizes import (NOISE, Problem, check_kappa, check_lml, check_posterior, kappa, kernel_with_noise, length_scale, lml_ref,
                            make_data)

pytestmark = pytest.mark.gpu

#: GPBO_ERR_STATE as a reader of an unfitted slot answers it (GPBO_ERR_HIP raises the same Python class: the message tells them apart)
UNFITTED = (_lib.GpboError, r"has not been fitted|is not fitted|run gpbo_posterior for slots")

#: worst error / bar per final state, written as JSON to the file GPBO_CALL_ORDER_REPORT names (if set) at the end of the module
WORST = {}


#: the library functions each scenario below runs as readers (module level, no engine call: the CPU cover test imports it)
SCENARIOS = {
    "A: the int8 digit planes of W": ("gpbo_posterior", "gpbo_lml_batch", "gpbo_get_L", "gpbo_get_K", "gpbo_get_Linv", "gpbo_get_alpha",
                                      "gpbo_predict_grad", "gpbo_acq_argbest"),
    "B: precision and size switches": ("gpbo_posterior",),
    "C: W^T in the K buffer": ("gpbo_polish_seeds", "gpbo_evolve_mixed", "gpbo_get_K", "gpbo_predict_cov", "gpbo_predict_grad",
                               "gpbo_lml_batch"),
    "D: unfitted means unfitted": ("gpbo_posterior", "gpbo_predict", "gpbo_predict_grad", "gpbo_predict_cov", "gpbo_polish_seeds",
                                   "gpbo_acq_argbest", "gpbo_get_L"),
    "E: candidates versus M_post": ("gpbo_posterior", "gpbo_acq_argbest", "gpbo_get_candidate_rows"),
    "F: the graph pool of gpbo_lml_batch": ("gpbo_lml_batch",),
    "G: the negative-variance flag": ("gpbo_take_negative_variance_flag", "gpbo_posterior", "gpbo_predict", "gpbo_predict_grad",
                                      "gpbo_predict_cov", "gpbo_polish_seeds", "gpbo_get_K", "gpbo_lml_batch", "gpbo_acq_argbest"),
}


def record(state, ratio):
    """`ratio`: an error over the bar it was just asserted against (the bar is named in `state`)."""
    WORST[state] = max(float(ratio), WORST.get(state, 0.0))


@pytest.fixture(scope="module", autouse=True)
def _call_order_report():
    yield
    import json

    out = os.environ.get("GPBO_CALL_ORDER_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump(dict(sorted(WORST.items())), f, indent=1)


# -- the replay helper ----------------------------------------------------------------------------------------------------
class Step:
    """One call: `method` an engine method's name (or a function of the engine), `kind` "w" (writer) or "r" (reader); `check`: the
    label its output is collected under; `name`: a label other steps can name in `needs` (reads the fresh side runs before them);
    `raises`: (exception class, message pattern) the call must answer with."""

    def __init__(self, kind, method, args, kw=None, check=None, name=None, needs=(), raises=None):
        self.kind, self.method, self.args, self.kw = kind, method, args, dict(kw or {})
        self.check, self.name, self.needs, self.raises = check, name or check, tuple(needs), raises


def W(method, *args, **opts):
    return Step("w", method, args, **opts)


def R(method, *args, **opts):
    return Step("r", method, args, **opts)


def _call(eng, s):
    fn = (lambda *a, **k: s.method(eng, *a, **k)) if callable(s.method) else getattr(eng, s.method)
    if s.raises is not None:
        with pytest.raises(s.raises[0], match=s.raises[1]):
            fn(*s.args, **s.kw)
        return None
    return fn(*s.args, **s.kw)


def replay(eng, steps):
    """Every step in order; {label: output} of the checked ones."""
    out = {}
    for s in steps:
        r = _call(eng, s)
        if s.check:
            out[s.check] = r
    return out


def replay_fresh(steps, debug=False, only=None):
    """{label: output} of every checked step (or of those in `only`), each from a fresh context of its own that ran the writers
    before the step, the reads it needs, and the step."""
    out = {}
    for i, s in enumerate(steps):
        if not s.check or (only is not None and s.check not in only):
            continue
        with GpEngine(0, debug=debug) as fresh:
            for t in steps[:i]:
                if t.kind == "w" or (t.name and t.name in s.needs):
                    _call(fresh, t)
            out[s.check] = _call(fresh, s)
    return out


def bits(x):
    """A value as something == compares bit for bit (-0.0 is not 0.0, a NaN equals the same NaN)."""
    if x is None:
        return None
    if isinstance(x, (tuple, list)):
        return tuple(bits(v) for v in x)
    a = np.asarray(x)
    return (a.dtype.str, a.shape, a.tobytes())


def assert_same_bits(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in want:
        assert bits(got[k]) == bits(want[k]), f"{what}: {k} differs from the fresh context's"


# -- shared builders ------------------------------------------------------------------------------------------------------
def _oracle(kernel, X, yn, ym, ys, ls, noise=NOISE):
    """(GPState in the targets' own units, kappa) of a from-scratch fit of the normalised targets."""
    K = O.kernel_matrix(kernel, X, None, ls)
    K[np.diag_indices_from(K)] += noise
    L = cholesky(K, lower=True)
    return O.GPState(kernel, np.atleast_1d(ls), noise, X, L, cho_solve((L, True), yn), ym, ys), kappa(K, L)


def _search_problem(N, d, seed):
    """test_gpu_polish_fused.py's problem: uniform inputs, a sine of their sum, length scale 0.25 sqrt(d)."""
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(N, d))
    y = np.sin(3 * X.sum(1)) + 0.05 * rng.randn(N)
    return X, y, 0.25 * np.sqrt(d)


@pytest.fixture
def post_kernel():
    """GPBO_POST_KERNEL for one pass (read per call by the debug build only), always removed again."""
    def run(eng, path, *args):
        os.environ["GPBO_POST_KERNEL"] = path
        try:
            return eng.posterior(*args)
        finally:
            os.environ.pop("GPBO_POST_KERNEL", None)

    os.environ.pop("GPBO_POST_KERNEL", None)
    yield run
    os.environ.pop("GPBO_POST_KERNEL", None)


A_N0, A_D, A_M = 2040, 5, 384          # NP = 2048 = I8_NP_MIN; the GEMV limit there is 256


def _problem_a(seed=61):
    """2044 rows (NP stays 2048 through the appends) and 384 candidates, 16 of them within 1e-3 of the four rows that get appended."""
    X, y, Xc = make_data(A_N0 + 4, A_D, seed, M=A_M)
    rng = np.random.RandomState(seed + 1)
    for i in range(16):
        u = rng.standard_normal(A_D)
        Xc[i] = np.clip(X[A_N0 + i % 4] + 0.9e-3 * u / np.linalg.norm(u), 0.0, 1.0)
    return X, y, Xc, length_scale(O.MATERN25, A_D, False, A_N0 + 4)


# -- A: the int8 digit planes of W ----------------------------------------------------------------------------------------
def test_int8_digit_planes_follow_every_writer(debug_engine, post_kernel):
    """NP = 2048, 384 candidates: fit, posterior (packs Wd), a ONE-row fit_append (the row-append kernel: W changes, NP does not),
    posterior, a three-row append, posterior + EI arg-best, a refit with the same X and new y (W unchanged: still exact), a refit with
    new X; gpbo_lml_batch, get_K, get_L, predict_grad as readers in between.  Every checked output is bitwise a fresh context's that
    did the writers only.  The model after each append is the oracle's (assert_same_model: K, L, W, alpha, mu, sd at its 1e-9
    Matern bar), the posterior after every later writer too (check_posterior, the same 1e-9).

    Observed, not assumed: the pass straight after the one-row append and the last one are bitwise the debug build's forced int8
    pass (GPBO_POST_KERNEL=8) and not its forced fp64 slab pass (=3) — PostPath::SlabI8; the one-row append ran the row-append
    kernel — its L is not the bits of a full fit of the same rows, which a rebuild's is (a 17-row append, one over the limit, is
    bitwise the full fit)."""
    eng, k = debug_engine, O.MATERN25
    X, y, Xc, ls = _problem_a()
    n0 = A_N0
    norm = {n: O.normalize_targets(y[:n]) for n in (n0, n0 + 1, n0 + 4)}
    y2 = np.cos(2.0 * X[:n0] @ np.linspace(0.5, 1.5, A_D)) + 0.05 * np.random.RandomState(5).standard_normal(n0)
    n2 = O.normalize_targets(y2)
    X3, y3, _ = make_data(n0, A_D, 67)
    n3 = O.normalize_targets(y3)
    y_max = float(y[:n0 + 4].max())
    Xs, ys_, ls_s = _search_problem(300, A_D, 3)
    lanes = np.array([[ls_s], [0.9 * ls_s], [1.1 * ls_s]])
    pts = Xc[:40]
    seen = {}

    def keep(label, fn):
        """A reader whose output the test looks at itself (the fresh side does not repeat it)."""
        return R(lambda e: seen.__setitem__(label, fn(e)))

    def reads(n, ym, ys):
        """Readers only; predict_grad leaves ITS points in the candidate buffer, so the step lists set the candidates again."""
        return [R("lml_batch", Xs, O.normalize_targets(ys_)[0], k, lanes, NOISE), keep(f"L {n}", lambda e: e.get_L(n)), R("get_K", n),
                R("predict_grad", pts, 0, ym, ys)]

    def forced(label, ym, ys):
        return [keep(f"{label} =8", lambda e: post_kernel(e, "8", 0, ym, ys)), keep(f"{label} =3", lambda e: post_kernel(e, "3", 0, ym, ys))]

    def same_model(n):
        yn, ym, ys = norm[n]
        return keep(f"model {n}", lambda e: assert_same_model(e, X[:n], yn, k, ls, NOISE, ym, ys, Xc))

    steps = [
        W("fit", X[:n0], norm[n0][0], k, ls, NOISE), W("set_candidates", Xc),
        R("posterior", 0, *norm[n0][1:], check="post fit"),
        *reads(n0, *norm[n0][1:]),
        W("fit_append", X[n0:n0 + 1], norm[n0 + 1][0]), W("set_candidates", Xc),
        R("posterior", 0, *norm[n0 + 1][1:], check="post append 1"),
        *forced("post append 1", *norm[n0 + 1][1:]),
        *reads(n0 + 1, *norm[n0 + 1][1:]), same_model(n0 + 1),
        W("fit_append", X[n0 + 1:n0 + 4], norm[n0 + 4][0]), W("set_candidates", Xc),
        R("posterior", 0, *norm[n0 + 4][1:], check="post append 3"),
        R("acq_argbest", O.EI, 0.01, y_max, kw=dict(k_seeds=16, return_values=True), check="ei append 3", needs=("post append 3",)),
        *reads(n0 + 4, *norm[n0 + 4][1:]), same_model(n0 + 4),
        W("fit", X[:n0], n2[0], k, ls, NOISE), W("set_candidates", Xc),
        R("posterior", 0, *n2[1:], check="post new y"),
        *reads(n0, *n2[1:]),
        W("fit", X3, n3[0], k, ls, NOISE), W("set_candidates", Xc),
        R("posterior", 0, *n3[1:], check="post new X"),
        *forced("post new X", *n3[1:]),
    ]
    got = replay(eng, steps)
    # the route, as test_gpu_int8_posterior.py establishes it: the default pass is the forced int8 pass, not the forced fp64 one
    for label in ("post append 1", "post new X"):
        (mu8, sd8), (mu3, sd3) = seen[f"{label} =8"], seen[f"{label} =3"]
        assert np.array_equal(got[label][0], mu8) and np.array_equal(got[label][1], sd8), f"{label}: the default at NP = 2048 is the int8 GEMM"
        assert np.array_equal(mu8, mu3) and not np.array_equal(sd8, sd3), f"{label}: GPBO_POST_KERNEL=3 takes another GEMM"
    assert_same_bits(got, replay_fresh(steps, debug=True), "int8 planes")
    # which kernel the appends ran
    with GpEngine(0, debug=True) as fresh:
        fresh.fit(X[:n0 + 1], norm[n0 + 1][0], k, ls, NOISE)
        assert not np.array_equal(seen[f"L {n0 + 1}"], fresh.get_L(n0 + 1)), "the one-row append rebuilt the factor"
        fresh.fit(X[:n0 + 4], norm[n0 + 4][0], k, ls, NOISE)
        L_full = fresh.get_L(n0 + 4)
        assert not np.array_equal(seen[f"L {n0 + 4}"], L_full), "the three-row append rebuilt the factor"
        fresh.fit(X[:n0 - 13], O.normalize_targets(y[:n0 - 13])[0], k, ls, NOISE)
        fresh.fit_append(X[n0 - 13:n0 + 4], norm[n0 + 4][0])
        assert np.array_equal(fresh.get_L(n0 + 4), L_full), "a rebuild (17 new rows) is bitwise the full fit"
    record("A SlabI8 after appends: assert_same_model, 1e-9 / 1e-7 / 1e-14", max(seen[f"model {n0 + 1}"], seen[f"model {n0 + 4}"]))
    worst = 0.0
    for label, n, Xn, (yn, ym, ys) in (("post append 1", n0 + 1, X, norm[n0 + 1]), ("post append 3", n0 + 4, X, norm[n0 + 4]),
                                       ("post new y", n0, X, n2), ("post new X", n0, X3, n3)):
        gp, kap = _oracle(k, Xn[:n], yn, ym, ys, ls)
        check_kappa(kap, label)
        mu_o, sd_o = O.predict(gp, Xc)
        worst = max(worst, check_posterior(*got[label], mu_o, sd_o, ys, f"{label} kappa={kap:.1e}"))
        if label == "post append 3":
            bi, bv, si, sv, vals = got["ei append 3"]
            vals_o = -1 * O.base_acq(O.EI, mu_o, sd_o, 0.01, y_max)
            order = np.argsort(vals_o, kind="stable")
            e = rel_err(vals, vals_o)
            assert e <= 1e-8 and bi == int(order[0]) and bv == vals[bi] and np.array_equal(si, order[:16]), (label, e)
            record("A EI values after appends: 1e-8", e / 1e-8)
    record("A SlabI8 mu / sd: check_posterior, 1e-9", worst)


# -- B: precision and size switches in one slot at int8 sizes -------------------------------------------------------------
def test_precision_and_size_switches_are_bitwise_a_fresh_fit(engine):
    """One slot: F64 at N = 2040, F32 of other data at the same N (Wp32 appears), F64 again, F64 at N = 2110 (NP = 2112: a ragged last
    chunk, the digit buffer grows), F64 at N = 1000 (below the int8 range, inside buffers that stay large), N = 2040 again.  Each
    posterior is bitwise the one of a fresh context that did only that fit, and the oracle's."""
    k, d = O.MATERN25, 5
    pa, pb = Problem(2040, k, d, False, M=A_M, seed=5), Problem(2040, k, d, False, M=A_M, seed=6)
    pc, pd = Problem(2110, k, d, False, M=A_M, seed=7), Problem(1000, k, d, False, M=A_M, seed=8)
    fresh, worst = {}, {"f64": 0.0, "f32": 0.0}
    for i, (p, prec) in enumerate(((pa, F64), (pb, F32), (pa, F64), (pc, F64), (pd, F64), (pa, F64))):
        steps = [W("fit", p.X, p.yn, k, p.ls, NOISE, kw=dict(precision=prec)), W("set_candidates", p.Xc),
                 R("posterior", 0, p.ym, p.ys, check="post")]
        got = replay(engine, steps)
        if (id(p), prec) not in fresh:
            fresh[(id(p), prec)] = replay_fresh(steps)
        assert_same_bits(got, fresh[(id(p), prec)], f"step {i}: {p.what} precision {prec}")
        check_kappa(p.kappa, p.what)
        mu, sd = got["post"]
        mu_o, sd_o = p.posterior(p.Xc)
        if prec == F32:
            e_mu, e_var = rel_err(mu, mu_o), float(np.max(np.abs(sd ** 2 - sd_o ** 2))) / p.ys ** 2
            assert e_mu < 1e-7 and e_var < 2e-5, f"step {i} {p.what} f32: mu {e_mu:.2e}, var {e_var:.2e}"
            worst["f32"] = max(worst["f32"], e_mu / 1e-7, e_var / 2e-5)
        else:
            worst["f64"] = max(worst["f64"], check_posterior(mu, sd, mu_o, sd_o, p.ys, f"step {i} {p.what}"))
    record("B f64 mu / sd: check_posterior, 1e-9", worst["f64"])
    record("B f32 mu 1e-7, variance 2e-5 (test_gpu_f32.py)", worst["f32"])


# -- C: W^T in the K buffer -----------------------------------------------------------------------------------------------
UCB_K = 2.576


def _polish(eng, ym, ys, seeds, box, max_iter=3):
    return eng.polish_seeds(O.UCB, UCB_K, 0.0, None, None, [ym], [ys], seeds, box, max_iter=max_iter)[:3]


def test_wt_in_the_k_buffer_survives_every_reader_of_k(debug_engine):
    """N = 300, d = 6 (NP = 320: the local searches stream W^T from the slot's K buffer).  Four searches with get_K, predict_cov,
    predict_grad and gpbo_lml_batch between them return the same bits, get_K is a fresh context's first get_K; then a one-row
    fit_append (the row-append kernel writes K), a search and get_K: the fresh context's that ran fit + append only.  The last
    search against the lockstep path and the oracle (_same_or_better), the last K against the oracle's."""
    eng, k, N, d = debug_engine, O.MATERN25, 300, 6
    X, y, ls = _search_problem(N + 1, d, 31)
    yn0, ym0, ys0 = O.normalize_targets(y[:N])
    yn1, ym1, ys1 = O.normalize_targets(y)
    rng = np.random.RandomState(9)
    seeds, pts = rng.uniform(size=(4, d)), rng.uniform(size=(40, d))
    box = np.array([[0.0, 1.0]] * d)
    lanes = np.array([[ls], [0.9 * ls], [1.15 * ls]])
    search0 = lambda e: _polish(e, ym0, ys0, seeds, box)
    search1 = lambda e: _polish(e, ym1, ys1, seeds, box)
    steps = [
        W("fit", X[:N], yn0, k, ls, NOISE),
        R(search0, check="search 1"), R("get_K", N, check="K"), R(search0, check="search 2"),
        R("predict_cov", pts, 0, ym0, ys0), R("predict_grad", pts, 0, ym0, ys0), R(search0, check="search 3"),
        R("lml_batch", X[:N], yn0, k, lanes, NOISE), R(search0, check="search 4"),
        W("fit_append", X[N:], yn1),
        R(search1, check="search after append"), R("get_K", N + 1, check="K after append"), R(search1, check="search after get_K"),
    ]
    got = replay(eng, steps)
    for i in (2, 3, 4):
        assert bits(got[f"search {i}"]) == bits(got["search 1"]), f"search {i} differs from the first"
    assert bits(got["search after get_K"]) == bits(got["search after append"])
    assert_same_bits(got, replay_fresh(steps, debug=True), "W^T at N = 300")
    # the final state: K, and the search against its checker (the lockstep path) and the oracle
    gp, kap = _oracle(k, X, yn1, ym1, ys1, ls)
    e_K = rel_err(got["K after append"], kernel_with_noise(k, X, ls))
    assert e_K < 1e-14, e_K
    os.environ["GPBO_POLISH_FUSED"] = "0"
    try:
        ref = search1(eng)
    finally:
        os.environ.pop("GPBO_POLISH_FUSED", None)
    _same_or_better(ref, got["search after get_K"], gp, O.UCB, UCB_K, 0.0)
    scale = max(abs(float(ref[1].min())), 1e-12)
    record("C WInMemory search against the lockstep path: _same_or_better, 1e-8", float(np.max(np.abs(got["search after get_K"][1] - ref[1]))) / (1e-8 * scale))
    record("C K after the append: 1e-14", e_K / 1e-14)


def _evolve(eng, ym, ys, y_max, groups, bounds, init, seed):
    rs = np.random.RandomState(seed)
    res = eng.evolve_mixed(O.UCB, UCB_K, y_max, ym, ys, groups, bounds, init, rs, maxiter=12)
    st = rs.get_state(legacy=True)
    return res + (st[1], st[2])


def test_wt_serves_the_evolution_and_w_in_lds_ignores_k(debug_engine):
    """The second consumer of W^T: gpbo_evolve_mixed on a two-float, one-integer space at N = 300 — get_K between two runs from the
    same RandomState copy: the same walk, result and stream position, a fresh context's too, the value the oracle's at the point.
    And the search / get_K / search core at N = 100 (NP = 128: W in LDS, K is never read): the history is invisible all the same."""
    eng, k = debug_engine, O.MATERN25
    rng = np.random.RandomState(17)
    N = 300
    X = np.column_stack([rng.uniform(size=(N, 2)), rng.randint(0, 5, size=N).astype(np.float64)])
    y = np.sin(3 * X[:, 0] + 2 * X[:, 1]) + 0.2 * X[:, 2] + 0.05 * rng.randn(N)
    yn, ym, ys = O.normalize_targets(y)
    ls = np.array([0.4, 0.4, 1.5])
    groups = [(0, 0, 1), (0, 1, 1), (1, 2, 1)]
    bounds = np.array([[0.0, 1.0], [0.0, 1.0], [0.0, 4.0]])
    init = bounds[:, 0] + (bounds[:, 1] - bounds[:, 0]) * rng.uniform(size=(45, 3))
    y_max = float(y.max())
    walk = lambda e: _evolve(e, ym, ys, y_max, groups, bounds, init, 8)
    steps = [W("fit", X, yn, k, ls, NOISE), R(walk, check="walk 1"), R("get_K", N), R(walk, check="walk 2")]
    got = replay(eng, steps)
    assert bits(got["walk 1"]) == bits(got["walk 2"]), "get_K changed the evolution"
    assert bits(replay_fresh(steps, debug=True, only=("walk 2",))["walk 2"]) == bits(got["walk 2"]), "evolution at N = 300: not a fresh context's"
    x, fun, nit, nfev = got["walk 2"][:4]
    gp, kap = _oracle(k, X, yn, ym, ys, ls)
    xt = x.copy()
    xt[2] = np.round(xt[2])
    f_at = float(O.neg_acquisition(gp, xt[None], O.UCB, UCB_K, y_max, None)[0])
    assert nit >= 1 and nfev > 45 and abs(fun - f_at) <= 1e-6 * abs(f_at) + 1e-9, (fun, f_at, nit, nfev)      # _same_or_better's last line
    record("C evolution value at its point: 1e-6", abs(fun - f_at) / (1e-6 * abs(f_at) + 1e-9))
    # W in LDS
    N, d = 100, 6
    X, y, ls = _search_problem(N, d, 37)
    yn, ym, ys = O.normalize_targets(y)
    seeds, box = np.random.RandomState(2).uniform(size=(4, d)), np.array([[0.0, 1.0]] * d)
    search = lambda e: _polish(e, ym, ys, seeds, box)
    steps = [W("fit", X, yn, k, ls, NOISE), R(search, check="search 1"), R("get_K", N, check="K"), R(search, check="search 2")]
    got = replay(eng, steps)
    assert bits(got["search 1"]) == bits(got["search 2"])
    assert_same_bits(got, replay_fresh(steps, debug=True), "W in LDS at N = 100")
    gp, kap = _oracle(k, X, yn, ym, ys, ls)
    os.environ["GPBO_POLISH_FUSED"] = "0"
    try:
        ref = search(eng)
    finally:
        os.environ.pop("GPBO_POLISH_FUSED", None)
    _same_or_better(ref, got["search 2"], gp, O.UCB, UCB_K, 0.0)
    assert rel_err(got["K"], kernel_with_noise(k, X, ls)) < 1e-14


# -- D: unfitted means unfitted -------------------------------------------------------------------------------------------
def _unfitted_reads(d, n):
    """Every reader of slot 0, each answering with the STATE error (n: the size get_L's array is made for)."""
    pts = np.random.RandomState(4).uniform(size=(8, d))
    box = np.array([[0.0, 1.0]] * d)
    return [R("posterior", 0, 0.0, 1.0, raises=UNFITTED), R("predict", pts, raises=UNFITTED), R("predict_grad", pts, raises=UNFITTED),
            R("predict_cov", pts, raises=UNFITTED),
            R("polish_seeds", O.UCB, UCB_K, 0.0, None, None, [0.0], [1.0], pts[:4], box, raises=UNFITTED),
            R("acq_argbest", O.EI, 0.01, 0.0, raises=UNFITTED), R("get_L", n, raises=UNFITTED)]


def test_an_unfitted_slot_raises_on_every_reader(engine):
    """A slot with cached digit planes (NP = 2048), then one with cached W^T (NP = 320): after gpbo_lml into the slot, and after a fit
    that is not positive definite (duplicate rows, RBF, no noise: a handled error code), every reader raises the STATE error — none
    serves the previous model's numbers — and a good fit afterwards is bitwise a fresh context's, and the oracle's."""
    k = O.MATERN25
    pa = Problem(A_N0, k, A_D, False, M=A_M, seed=9)
    fit_a = [W("fit", pa.X, pa.yn, k, pa.ls, NOISE), W("set_candidates", pa.Xc)]
    steps = fit_a + [R("posterior", 0, pa.ym, pa.ys),                                                # packs Wd
                     W("lml", pa.X, pa.yn, k, pa.ls, NOISE)] + _unfitted_reads(A_D, A_N0) + fit_a + \
        [R("posterior", 0, pa.ym, pa.ys, check="post")]
    got = replay(engine, steps)
    assert_same_bits(got, replay_fresh(steps), "after gpbo_lml at NP = 2048")
    check_kappa(pa.kappa, pa.what)
    record("D mu / sd after the good fit: check_posterior, 1e-9", check_posterior(*got["post"], *pa.posterior(pa.Xc), pa.ys, pa.what))

    N, d = 300, 6
    X, y, ls = _search_problem(N, d, 41)
    yn, ym, ys = O.normalize_targets(y)
    seeds, box = np.random.RandomState(6).uniform(size=(4, d)), np.array([[0.0, 1.0]] * d)
    Xc = np.random.RandomState(7).uniform(size=(200, d))
    search = lambda e: _polish(e, ym, ys, seeds, box)
    Xd = np.vstack([X[:150], X[:150]])
    steps = [W("fit", X, yn, k, ls, NOISE), R(search),                                                  # W^T into K
             W("lml", X, yn, k, ls, NOISE), *_unfitted_reads(d, N),
             W("fit", X, yn, k, ls, NOISE), R(search, check="search after lml"),
             W("fit", Xd, np.zeros(N), O.RBF, [1.0], 0.0, raises=(np.linalg.LinAlgError, "not returning a positive definite matrix")),
             *_unfitted_reads(d, N),
             W("fit_append", X[:1], np.zeros(N + 1), raises=(_lib.GpboError, "no fitted model")), *_unfitted_reads(d, N),
             W("fit", X, yn, k, ls, NOISE), W("set_candidates", Xc),
             R(search, check="search after not PD"), W("set_candidates", Xc), R("posterior", 0, ym, ys, check="post after not PD")]
    got = replay(engine, steps)
    assert bits(got["search after lml"]) == bits(got["search after not PD"])
    assert_same_bits(got, replay_fresh(steps), "after gpbo_lml and a failed fit at NP = 320")
    gp, kap = _oracle(k, X, yn, ym, ys, ls)
    mu_o, sd_o = O.predict(gp, Xc)
    record("D mu / sd after the good fit: check_posterior, 1e-9", check_posterior(*got["post after not PD"], mu_o, sd_o, ys, f"N=300 kappa={kap:.1e}"))


# -- E: candidates versus M_post, two slots -------------------------------------------------------------------------------
def test_stale_posteriors_are_refused_not_used(engine):
    """Constrained EI over slots 0 (N = 150) and 1 (N = 2040): after a refit of slot 1 alone, and after new candidates, gpbo_acq_argbest
    raises the STATE error until the posteriors it reads are redone — it never multiplies by the old sigma — and then equals the
    fresh context's and the oracle's.  transform_candidates keeps get_candidate_rows returning the rows as drawn, and the posterior
    behind it sees the transformed ones."""
    k, d = O.MATERN25, 5
    p0, p1 = Problem(150, k, d, False, M=A_M, seed=11), Problem(A_N0, k, d, False, M=A_M, seed=12)
    rng = np.random.RandomState(13)
    c2 = np.cos(3.0 * p1.X @ rng.uniform(0.5, 1.5, d)) + 0.05 * rng.standard_normal(A_N0)
    c2n, c2m, c2s = O.normalize_targets(c2)
    Xc, Xc2 = p0.Xc, rng.uniform(size=(200, d))
    Xc3 = np.column_stack([rng.uniform(size=(210, d - 1)), rng.uniform(-0.4, 1.4, size=210)])
    groups = [(0, 0, d - 1), (1, d - 1, 1)]
    idx = np.array([0, 7, 209])
    y_max, ub = float(np.median(p0.y)), float(np.median(p1.y))
    acq = dict(kw=dict(k_seeds=16, return_values=True))
    args = (O.EI, 0.01, y_max, [-np.inf], [ub])
    stale = (_lib.GpboError, "run gpbo_posterior for slots")
    post0, post1, post1b = ("posterior", 0, p0.ym, p0.ys), ("posterior", 1, p1.ym, p1.ys), ("posterior", 1, c2m, c2s)
    steps = [
        W("fit", p0.X, p0.yn, k, p0.ls, NOISE), W("fit", p1.X, p1.yn, k, p1.ls, NOISE, kw=dict(slot=1)), W("set_candidates", Xc),
        R(*post0, name="p0"), R(*post1, kw=dict(fetch=False), name="p1"), R("acq_argbest", *args, **acq, check="acq", needs=("p0", "p1")),
        W("fit", p1.X, c2n, k, p1.ls, NOISE, kw=dict(slot=1)),
        R("acq_argbest", *args, raises=stale),
        R(*post1b, kw=dict(fetch=False), name="p1b"), R("acq_argbest", *args, **acq, check="acq refit", needs=("p0", "p1b")),
        W("set_candidates", Xc2),
        R("acq_argbest", *args, raises=stale), R(*post0, name="p0c"), R("acq_argbest", *args, raises=stale),
        R(*post1b, name="p1c"), R("acq_argbest", *args, **acq, check="acq new candidates", needs=("p0c", "p1c")),
        W("set_candidates", Xc3), W("transform_candidates", groups),
        R("acq_argbest", *args, raises=stale), R("get_candidate_rows", idx, d, check="rows"),
        R(*post0, name="p0t"), R(*post1b, name="p1t"), R("acq_argbest", *args, **acq, check="acq transformed", needs=("p0t", "p1t")),
    ]
    got = replay(engine, steps)
    assert np.array_equal(got["rows"], Xc3[idx]), "get_candidate_rows returns the rows as drawn"
    assert_same_bits(got, replay_fresh(steps), "two slots")
    gp1, kap1 = _oracle(k, p1.X, c2n, c2m, c2s, p1.ls)
    check_kappa(p0.kappa, p0.what), check_kappa(kap1, "slot 1")
    Xt = Xc3.copy()
    Xt[:, d - 1] = np.round(Xt[:, d - 1])
    worst = 0.0
    for label, cand, cgp in (("acq", Xc, p1.gp()), ("acq refit", Xc, gp1), ("acq new candidates", Xc2, gp1), ("acq transformed", Xt, gp1)):
        bi, bv, si, sv, vals = got[label]
        vals_o = O.neg_acquisition(p0.gp(), cand, O.EI, 0.01, y_max, ([cgp], [-np.inf], [ub]))
        order = np.argsort(vals_o, kind="stable")
        e = rel_err(vals, vals_o)
        assert e <= 1e-8 and bi == int(order[0]) and bv == vals[bi] and np.array_equal(si, order[:16]), (label, e, bi, order[:3])
        worst = max(worst, e / 1e-8)
    record("E constrained EI values: 1e-8", worst)


# -- F: the graph pool of gpbo_lml_batch ----------------------------------------------------------------------------------
def test_lml_batch_graph_pool_replacement_and_recapture(engine):
    """N = 800 (NP = 832: the Blocked tier, the graph-eligible one), 3 lanes, 26 keys = 13 noise values x eval_gradient: each key twice
    (the second sighting of a key is the one that captures: 24 keys fill the pool of LML_GRAPH_POOL = 24, two more replace the least
    recently used), then all 26 again in the same order — under least-recently-used replacement each has been replaced by then, so
    each is a first sighting and a capture once more.  What is asserted is what a caller can see: every value and gradient of all
    104 calls is bitwise gpbo_lml's, three keys are the oracle's, and reuse_inputs after a call of another shape is the STATE error.
    Whether a call replayed a graph is NOT visible through the ABI: a context whose capture failed once launches directly from then
    on (lml_graph_off), and on such a context this test checks the direct launches under the same sequence of keys and no more."""
    k, N, d = O.MATERN25, 800, 4
    X, y, _ = make_data(N, d, 71)
    yn = O.normalize_targets(y)[0]
    ls0 = 0.2 * np.sqrt(d)
    lanes = np.array([[ls0], [0.93 * ls0], [1.09 * ls0]])
    noises = [1e-6 * (1.0 + 0.25 * i) for i in range(13)]
    keys = [(nz, eg) for nz in noises for eg in (0, 1)]
    assert len(keys) == 26 > 24
    want = {}
    for nz, eg in keys:
        for row in lanes:
            r = engine.lml(X, yn, k, row, nz, eval_gradient=bool(eg))
            want[(nz, eg, float(row[0]))] = (r[0], r[1].copy()) if eg else (r, np.zeros(1))
    got = {}
    for rnd in range(2):
        for nz, eg in keys:
            for rep in range(2):
                vals, grads = engine.lml_batch_arrays(X, yn, k, lanes, nz, eval_gradient=bool(eg))
                for i, row in enumerate(lanes):
                    v, g = want[(nz, eg, float(row[0]))]
                    what = f"round {rnd} noise {nz:.3e} eval_gradient {eg} sighting {rep} lane {i}"
                    assert vals[i] == v and np.isfinite(v), what
                    assert np.array_equal(grads[i], g), what
                got[(nz, eg)] = (vals.copy(), grads.copy())
    worst = 0.0
    for nz in (noises[0], noises[6], noises[12]):
        for i, row in enumerate(lanes):
            K = O.kernel_matrix(k, X, None, row)
            K[np.diag_indices_from(K)] += nz
            L = cholesky(K, lower=True)
            kap = kappa(K, L)
            check_kappa(kap, f"noise {nz:.2e} lane {i}")
            lml_o, grad_o = lml_ref(k, X, yn, row, L)
            worst = max(worst, check_lml(got[(nz, 1)][0][i], got[(nz, 1)][1][i], lml_o, grad_o, f"noise {nz:.2e} lane {i} kappa={kap:.1e}"))
            e_v = abs(got[(nz, 0)][0][i] - lml_o) / max(1.0, abs(lml_o))
            assert e_v <= 1e-10, (nz, i, e_v)
    # resident inputs of another shape
    X9, y9, _ = make_data(900, d, 72)
    engine.lml_batch(X9, O.normalize_targets(y9)[0], k, lanes, NOISE)
    with pytest.raises(_lib.GpboError, match="no resident inputs of this shape"):
        engine.lml_batch(X, yn, k, lanes, NOISE, reuse_inputs=True)
    vals, grads = engine.lml_batch_arrays(X, yn, k, lanes, noises[3])      # and the pool still answers
    assert all(vals[i] == want[(noises[3], 1, float(row[0]))][0] for i, row in enumerate(lanes))
    record("F Blocked LML and gradient: check_lml, 1e-10 / 1e-7", worst)


# -- G: the negative-variance flag ----------------------------------------------------------------------------------------
def test_negative_variance_flag_is_set_by_clips_and_cleared_by_taking_it(engine):
    """include/gpbo.h: the flag reports whether any gpbo_posterior / gpbo_predict / gpbo_predict_grad since the last take clipped a
    NEGATIVE variance, and taking it clears it; the one-launch search stores to the same word.  All four are made to clip here, and
    after each one take answers True and the next take False.

    posterior, predict: the inputs of test_predict_warns_on_negative_variances_only_like_sklearn — the fp32 posterior at the training
    points of a model with noise 1e-8 clips, the fp64 one does not.  predict_grad and the search read the fp64 W whatever the fit's
    precision, so they need an fp64 model whose variance at a training point is below the rounding of 1 - |W k*|^2: the first 300
    rows of the same inputs with noise 1e-15, queried ON training rows.  There the true variance is ~ 1e-15 < 2^-53 and the sign of
    the computed one is rounding alone: 54 of the first 256 rows clip in predict_grad (13 of 100 at N = 100), so that none of 64
    seeds clips is not a knife edge; these passes are bitwise repeatable, so which rows clip is fixed.  N = 300 is the search's
    W-in-memory kernel, N = 100 its W-in-LDS one.

    Readers of a well-conditioned model in between — posterior, predict, predict_grad, predict_cov, the one-launch search, get_K,
    gpbo_lml_batch, the arg-best — neither set nor clear it, and neither do the writers."""
    k = O.MATERN25
    rs = np.random.RandomState(3)
    X = rs.uniform(size=(600, 3))
    yn, ym, ys = O.normalize_targets(np.sin(3 * X.sum(axis=1)))
    Xq = np.concatenate([X] * 3)
    Xw, yw, lw = _search_problem(300, 3, 43)
    ywn, ywm, yws = O.normalize_targets(yw)
    pts = np.random.RandomState(5).uniform(size=(60, 3))
    box = np.array([[0.0, 1.0]] * 3)

    def clip(how, n=300):
        """One clipping call of the kind `how`; True when its output shows the clip (the search returns no deviation)."""
        if how in ("posterior", "predict"):
            engine.fit(X, yn, k, 0.7, 1e-8, precision=F32)
            if how == "posterior":
                engine.set_candidates(Xq)
                return bool((engine.posterior(0, ym, ys)[1] == 0).any())
            return bool((engine.predict(Xq, y_mean=ym, y_std=ys)[1] == 0).any())
        y3n, y3m, y3s = O.normalize_targets(np.sin(3 * X[:n].sum(axis=1)))
        engine.fit(X[:n], y3n, k, 0.7, 1e-15)
        assert engine.take_negative_variance_flag() is False, "a fit set the flag"
        if how == "predict_grad":
            mu, sd, dmu, dsd = engine.predict_grad(X[:min(n, 256)], 0, y3m, y3s)
            clipped = sd == 0
            assert np.all(dsd[clipped] == 0), "a clipped variance has no slope"
            return bool(clipped.any())
        _polish(engine, y3m, y3s, X[:64], box)
        return True

    def well_conditioned_reads():
        engine.fit(Xw, ywn, k, lw, NOISE)
        engine.predict(pts, y_mean=ywm, y_std=yws)
        engine.acq_argbest(O.UCB, UCB_K)
        engine.predict_grad(pts, 0, ywm, yws)
        engine.predict_cov(pts, 0, ywm, yws)
        _polish(engine, ywm, yws, pts[:4], box)
        engine.get_K(300)
        engine.lml_batch(Xw, ywn, k, np.array([[lw], [1.1 * lw]]), NOISE)
        engine.set_candidates(np.vstack([pts] * 5))
        engine.posterior(0, ywm, yws)

    engine.take_negative_variance_flag()
    well_conditioned_reads()
    assert engine.take_negative_variance_flag() is False, "a reader of a well-conditioned model set the flag"
    engine.fit(X, yn, k, 0.7, 1e-8)                     # fp64 on the ill-conditioned model: no clip, no flag
    sd64 = engine.predict(Xq, y_mean=ym, y_std=ys)[1]
    assert not (sd64 == 0).any() and engine.take_negative_variance_flag() is False
    for how, n in (("posterior", 600), ("predict", 600), ("predict_grad", 300), ("predict_grad", 100), ("search", 300), ("search", 100)):
        assert clip(how, n), (how, n)
        assert engine.take_negative_variance_flag() is True, f"{how} at N = {n} clipped and did not set the flag"
        assert engine.take_negative_variance_flag() is False, "taking the flag clears it"
    for how in ("posterior", "predict_grad", "search"):
        clip(how)
        well_conditioned_reads()
        assert engine.take_negative_variance_flag() is True, f"a reader or a writer in between cleared the flag {how} had set"
        assert engine.take_negative_variance_flag() is False
    well_conditioned_reads()
    assert engine.take_negative_variance_flag() is False
