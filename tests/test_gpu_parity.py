"""GPU (-m gpu): the HIP path, called through the C ABI, against the CPU oracle on the same seeded
inputs.  Tolerances: north_star asks 1e-5 relative in fp64 with the arg-best index exact; the HIP
path actually lands at <= 1e-9, which is what is asserted (max-norm relative, stated per test)."""
import numpy as np
import pytest

from bayesianoptimization_amd import _lib
from bayesianoptimization_amd import workloads as W
from conftest import rel_err
from helpers import assert_same_model as _assert_same_model
from helpers import oracle_case
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _data(N, d, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(N, d))
    y = np.sin(3 * X.sum(1)) + 0.1 * rng.randn(N)
    return X, y


@pytest.mark.parametrize("m,n,k,bt", [(64, 64, 16, False), (128, 192, 64, False), (192, 64, 48, True), (64, 128, 32, True),
                                      # the 128x128 double-buffered kernel (m, n >= 128, k >= 32), incl. ragged last blocks
                                      (128, 128, 32, True), (256, 384, 512, True), (320, 192, 80, False),
                                      (448, 704, 144, True), (192, 192, 48, False)])
def test_mfma_gemm_layout(debug_engine, m, n, k, bt):
    engine = debug_engine      # gpbo_debug_gemm: debug build
    """Transpose-detecting check of the f64 MFMA fragment maps (asymmetric random operands)."""
    rng = np.random.RandomState(1)
    A = rng.randn(m, k)
    B = rng.randn(n, k) if bt else rng.randn(k, n)
    C0 = rng.randn(m, n)
    got = engine.debug_gemm(A, B, C0, alpha=0.5, beta=-2.0, b_trans=bt)
    ref = 0.5 * (A @ (B.T if bt else B)) - 2.0 * C0
    assert rel_err(got, ref) < 1e-13


@pytest.mark.parametrize("N,d,kernel,ls", [
    (1, 1, O.MATERN25, 0.5), (2, 2, O.RBF, 0.7), (63, 3, O.MATERN25, 0.4), (64, 5, O.MATERN25, 0.6),
    (65, 8, O.RBF, 0.9), (200, 16, O.MATERN25, 1.2), (257, 17, O.MATERN25, 1.5), (320, 32, O.RBF, 2.0),
    (130, 40, O.MATERN25, 2.5), (100, 4, O.MATERN25, [0.3, 0.5, 0.8, 1.1]),
])
def test_fit_parity(engine, N, d, kernel, ls):
    """K (kernels.py:1711-1738), L (_gpr.py:349), W = L^-1, alpha (_gpr.py:360-364) vs the oracle."""
    X, y = _data(N, d)
    gp = O.fit_fixed_theta(kernel, X, y, ls, 1e-6)
    yn, _, _ = O.normalize_targets(y)
    engine.fit(X, yn, kernel, ls, 1e-6)
    K = O.kernel_matrix(kernel, X, None, ls)
    K[np.diag_indices_from(K)] += 1e-6
    assert rel_err(engine.get_K(N), K) < 1e-14
    assert rel_err(engine.get_L(N), gp.L) < 1e-10
    assert rel_err(engine.get_Linv(N), np.linalg.inv(gp.L)) < 1e-8
    assert rel_err(engine.get_alpha(N), gp.alpha) < 1e-8
    Lg = engine.get_L(N)
    assert np.all(np.triu(Lg, 1) == 0.0)
    assert rel_err(Lg @ Lg.T, K) < 1e-13


@pytest.mark.parametrize("kernel", [O.MATERN25, O.RBF])
def test_kernel_value_exp_against_numpy(engine, kernel):
    """gpbo_kernel_value's own exp (gpbo_exp_nonpos: Cody-Waite reduction + degree-13 polynomial + v_ldexp_f64, round 4) over the whole
    range a kernel matrix can reach: points on a line give exponents from 0 down to below the subnormals.  Against NumPy's exp of
    the same argument: relative error <= 4e-16 (1 + |argument|) wherever the value is a normal number (the argument itself carries
    one rounding, which exp magnifies by |argument| — for any implementation), absolute error <= one subnormal step below, exactly
    1 + noise on the diagonal, exactly 0 where NumPy underflows to 0, and never a NaN."""
    N = 320
    rng = np.random.RandomState(9)
    pos = np.sort(np.concatenate([[0.0], rng.uniform(0, 1, 99), rng.uniform(1, 30, 120), rng.uniform(30, 420, 100)]))
    X = pos[:, None]
    yn = rng.standard_normal(N)
    engine.fit(X, yn, kernel, 1.0, 1e-6)
    K = engine.get_K(N)
    r = np.abs(pos[:, None] - pos[None, :])
    if kernel == O.MATERN25:
        k = np.sqrt(5.0) * r
        arg, ref = -k, (1.0 + k + k * k / 3.0) * np.exp(-k)
    else:
        arg = -0.5 * r * r
        ref = np.exp(arg)
    ref[np.diag_indices(N)] += 1e-6
    assert np.all(np.isfinite(K))
    assert np.array_equal(np.diag(K), np.full(N, 1.0 + 1e-6))
    normal = ref > 2.3e-308
    assert arg.min() < -760 and np.sum(~normal) > 100          # the sample reaches the subnormals and exact zero
    rel = np.abs(K - ref)[normal] / ref[normal]
    assert np.max(rel / (1.0 + np.abs(arg[normal]))) < 4e-16
    assert np.max(np.abs(K - ref)[~normal]) <= 1e-307 * 4e-16 + 5e-324 * 2 ** 12
    assert np.all(K[ref == 0.0] == 0.0)


def test_kernel_value_exp_extreme_arguments(engine):
    """gpbo_exp_nonpos beyond the range a sane kernel matrix reaches.  RBF entries of points 1e150 (squared distance
    1e300) and 1e200 apart (squared distance overflows to +inf): NumPy's exp gives exactly 0 for both; the device's reduction
    used to give NaN for -inf (inf - inf) and garbage beyond |x| ~ 1e40."""
    X = np.array([[0.0], [1.0], [1e150], [1e200], [-1e200]])
    yn = np.array([0.3, -0.2, 0.1, 0.5, -0.4])
    engine.fit(X, yn, O.RBF, 1.0, 1e-6)
    K = engine.get_K(5)
    with np.errstate(over="ignore"):
        ref = np.exp(-0.5 * (X - X.T) ** 2)
    ref[np.diag_indices(5)] = 1.0 + 1e-6
    assert np.all(np.isfinite(K))
    assert np.array_equal(K[2:, :2], np.zeros((3, 2))) and K[3, 2] == 0.0 and K[4, 3] == 0.0
    assert np.allclose(K, ref, rtol=1e-15, atol=0.0)
    mu, sd = engine.predict(np.array([[0.5], [1e180], [np.inf]]))        # k* rows of zeros: the prior
    assert np.isfinite(mu[:2]).all() and mu[1] == 0.0 and sd[1] == 1.0
    assert np.isnan(mu[2]) or mu[2] == 0.0                                 # inf - inf inside the distance: NaN, as NumPy's cdist


@pytest.mark.parametrize("M", [1, 2, 127, 128, 129, 1000, 4097])
def test_posterior_parity_ragged_candidate_counts(engine, M):
    X, y = _data(150, 6, seed=2)
    gp = O.fit_fixed_theta(O.MATERN25, X, y, 0.8, 1e-6)
    yn, ym, ys = O.normalize_targets(y)
    engine.fit(X, yn, O.MATERN25, 0.8, 1e-6)
    Xc = np.random.RandomState(3).uniform(size=(M, 6))
    mu, sd = engine.predict(Xc, y_mean=ym, y_std=ys)
    mu_o, sd_o = O.predict(gp, Xc)
    assert mu.shape == (M,) and sd.shape == (M,)
    assert rel_err(mu, mu_o) < TOL and rel_err(sd, sd_o) < TOL


@pytest.mark.parametrize("name,ls,cls", [("P1", 0.4, None), ("P2", 0.6, None), ("C5S", 0.5, 0.7)])
def test_acquisition_and_argbest_parity(engine, name, ls, cls):
    """-acq [* p_c], argmin, min, argsort[:k] (acquisition.py:198-217, 312-317; constraint.py:199-221)."""
    w = W.ALL[name]
    oc = oracle_case(w, ls, c_length_scale=cls)
    yn, ym, ys_ = O.normalize_targets(oc["y"])
    engine.fit(oc["X"], yn, w.kernel, ls, w.noise, slot=0)
    engine.set_candidates(oc["Xc"])
    mu, sd = engine.posterior(0, ym, ys_)
    lb = ub = None
    if w.constrained:
        cn, cm, cs = O.normalize_targets(oc["c"])
        engine.fit(oc["X"], cn, W.MATERN25, cls, w.noise, slot=1)
        engine.posterior(1, cm, cs, fetch=False)
        lb, ub = [-np.inf], [w.constraint_ub]
    for acq, param in [(w.acq, w.acq_param), (W.UCB, 2.576), (W.EI, 0.0), (W.POI, 0.05)]:
        if w.constrained and acq == W.UCB:
            continue  # the reference refuses UCB with constraints (acquisition.py:524-529)
        ys_o = O.neg_acquisition(oc["gp"], oc["Xc"], acq, param, oc["y_max"], oc["cons"])
        bi, bv, si, sv, ys = engine.acq_argbest(acq, param, oc["y_max"], lb, ub, k_seeds=12, return_values=True)
        scale = np.max(np.abs(ys_o))
        # RBF Gram matrices are far worse conditioned than Matern ones (P2: kappa(K) ~ 1e9 at alpha=1e-6),
        # and both LAPACK and the device carry ~kappa*eps of rounding noise: 1e-7 there, 1e-9 otherwise.
        tol = 1e-7 if w.kernel == W.RBF else TOL
        assert np.max(np.abs(ys - ys_o)) <= tol * scale
        oi, ov, os_ = O.arg_best(ys_o, 12)
        assert bi == oi
        assert bv == ys[bi] and np.array_equal(sv, ys[si])
        # argsort(ys)[:k]: identical indices unless values tie exactly (POI saturates at -1.0 on confident
        # posteriors); NumPy's introsort leaves the order of equal keys unspecified, the device breaks ties
        # by lowest index — so compare the selected VALUES always and the indices when the keys are distinct.
        srt = np.sort(ys_o)
        assert np.allclose(sv, srt[:12], rtol=tol, atol=tol * scale)
        if np.all(np.diff(srt[:13]) > 4 * tol * scale):
            assert np.array_equal(si, os_)
        else:
            nan = np.isnan(ys)
            assert np.array_equal(si, np.lexsort((np.arange(len(ys)), np.where(nan, np.inf, ys), nan))[:12])


def test_two_sided_and_multiple_constraints(engine):
    rng = np.random.RandomState(4)
    X = rng.uniform(size=(90, 3))
    y = np.sin(3 * X.sum(1))
    c1, c2 = np.cos(2 * X.sum(1)), X[:, 0] - X[:, 1]
    gps = [O.fit_fixed_theta(O.MATERN25, X, t, ls, 1e-6) for t, ls in ((y, 0.5), (c1, 0.7), (c2, 0.9))]
    for s, (t, ls) in enumerate(((y, 0.5), (c1, 0.7), (c2, 0.9))):
        tn, tm, ts = O.normalize_targets(t)
        engine.fit(X, tn, O.MATERN25, ls, 1e-6, slot=s)
    Xc = rng.uniform(size=(3000, 3))
    engine.set_candidates(Xc)
    for s, t in enumerate((y, c1, c2)):
        _, tm, ts = O.normalize_targets(t)
        engine.posterior(s, tm, ts, fetch=False)
    lb, ub = [-0.2, -np.inf], [0.6, 0.1]
    ys_o = O.neg_acquisition(gps[0], Xc, O.EI, 0.01, y.max(), (gps[1:], lb, ub))
    bi, bv, si, sv, ys = engine.acq_argbest(O.EI, 0.01, y.max(), lb, ub, k_seeds=5, return_values=True)
    assert np.max(np.abs(ys - ys_o)) <= TOL * np.max(np.abs(ys_o))
    assert bi == int(ys_o.argmin()) and np.array_equal(si, np.argsort(ys_o)[:5])


def test_nan_and_tie_semantics(engine):
    """numpy argmin: first NaN wins; argsort: NaNs last; ties -> lowest index (SURVEY.md §7 'Arg-best')."""
    X, y = _data(40, 2, seed=5)
    yn, ym, ys_ = O.normalize_targets(y)
    engine.fit(X, yn, O.RBF, 0.5, 1e-6)
    Xc = np.random.RandomState(6).uniform(size=(600, 2))
    Xc[[77, 300]] = np.nan                      # NaN inputs -> NaN posterior -> NaN acquisition
    Xc[401] = Xc[17]
    Xc[555] = Xc[17]                            # exact duplicates -> exact ties
    engine.set_candidates(Xc)
    engine.posterior(0, ym, ys_, fetch=False)
    bi, bv, si, sv, ys = engine.acq_argbest(O.UCB, 1.0, k_seeds=64, return_values=True)
    assert np.isnan(ys[77]) and np.isnan(ys[300]) and ys[401] == ys[17] == ys[555]
    assert bi == 77 and np.isnan(bv)
    assert bi == int(np.argmin(ys))
    nan = np.isnan(ys)
    order = np.lexsort((np.arange(600), np.where(nan, np.inf, ys), nan))
    assert np.array_equal(si, order[:64])
    pos = {int(i): p for p, i in enumerate(order)}
    assert pos[17] < pos[401] < pos[555]
    # more seeds than candidates: padded with -1
    engine.set_candidates(Xc[:5])
    engine.posterior(0, ym, ys_, fetch=False)
    bi, bv, si, sv, _ = engine.acq_argbest(O.UCB, 1.0, k_seeds=8)
    assert list(si[5:]) == [-1, -1, -1] and sorted(si[:5]) == [0, 1, 2, 3, 4]


def test_sigma_zero_conventions(engine):
    """sd = 0 exactly (clipped variance): EI -> a / 0 / NaN, POI -> 1 / 0 / NaN, as NumPy."""
    X = np.array([[0.25], [0.75]])
    y = np.array([0.0, 1.0])
    engine.fit(X, y, O.RBF, 1.0, 0.0)           # noise-free: sd at a training point is exactly 0 or ~1e-8
    engine.set_candidates(X)
    mu, sd = engine.posterior(0, 0.0, 1.0)
    gp = O.fit_fixed_theta(O.RBF, X, y, 1.0, 0.0, normalize_y=False)
    mu_o, sd_o = O.predict(gp, X)
    for acq in (O.EI, O.POI):
        _, _, _, _, ys = engine.acq_argbest(acq, 0.0, y_max=1.0, return_values=True)
        with np.errstate(all="ignore"):
            ref = -1 * O.base_acq(acq, mu, sd, 0.0, 1.0)    # same formulas on the device's own mu/sd
        assert np.array_equal(ys, ref, equal_nan=True)


def test_not_positive_definite_raises_linalgerror(engine):
    X = np.array([[0.1, 0.2], [0.1, 0.2], [0.5, 0.5]])   # duplicate rows, no jitter
    with pytest.raises(np.linalg.LinAlgError, match="not returning a positive definite matrix"):
        engine.fit(X, np.zeros(3), O.MATERN25, 1.0, 0.0)
    # the context stays usable
    engine.fit(X, np.zeros(3), O.MATERN25, 1.0, 1e-6)


def test_error_codes_map_to_python_exceptions(engine):
    X, y = _data(10, 2)
    with pytest.raises(NotImplementedError):
        engine.fit(X, y, 7, 1.0, 1e-6)                      # unknown kernel
    with pytest.raises(NotImplementedError):
        engine.fit(X, y, O.RBF, 1.0, 1e-6, precision=7)     # unknown precision enum
    with pytest.raises(ValueError):
        engine.fit(X, y, O.RBF, [1.0, 2.0, 3.0], 1e-6)      # wrong length_scale size
    with pytest.raises(ValueError):
        engine.fit(X, y, O.RBF, -1.0, 1e-6)
    with pytest.raises(_lib.GpboError):
        engine.posterior(5)                                  # slot never fitted
    engine.fit(X, y, O.RBF, 1.0, 1e-6)
    engine.set_candidates(np.zeros((4, 3)))
    with pytest.raises(ValueError):
        engine.posterior(0)                                  # candidate dimension mismatch
    engine.set_candidates(np.zeros((4, 2)))
    with pytest.raises(_lib.GpboError):
        engine.acq_argbest(O.UCB, 1.0)                       # posterior not run for these candidates
    with pytest.raises(ValueError):
        engine.set_candidates(np.zeros((0, 2)))              # empty candidate set (the host handles n_random == 0)
    with pytest.raises(ValueError):
        engine.fit(np.zeros((0, 2)), np.zeros(0), O.RBF, 1.0, 1e-6)   # no observations
    with pytest.raises(NotImplementedError):
        engine.fit(np.zeros((3, 65)), np.zeros(3), O.RBF, 1.0, 1e-6)  # d > 64


def test_bitwise_determinism(engine):
    w = W.P1
    oc = oracle_case(w, 0.4)
    yn, ym, ys_ = O.normalize_targets(oc["y"])
    outs = []
    for _ in range(3):
        engine.fit(oc["X"], yn, w.kernel, 0.4, w.noise)
        engine.set_candidates(oc["Xc"])
        mu, sd = engine.posterior(0, ym, ys_)
        bi, bv, si, sv, ys = engine.acq_argbest(O.EI, 0.01, oc["y_max"], k_seeds=10, return_values=True)
        outs.append((engine.get_L(w.N), mu, sd, ys, bi, tuple(si)))
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(o[:4], outs[0][:4]))
        assert o[4:] == outs[0][4:]


def test_event_records_can_be_switched_off_and_change_no_result(engine):
    """gpbo_set_timing(ctx, 0): the calls stop recording their HIP event pairs (marker packets on the stream: 28 us of a
    119 us step of BASELINE config 1), gpbo_last_timings answers -1, every result keeps its bits; 1 brings the timings back."""
    w = W.P1
    oc = oracle_case(w, 0.4)
    yn, ym, ys_ = O.normalize_targets(oc["y"])

    def run():
        engine.fit(oc["X"], yn, w.kernel, 0.4, w.noise)
        engine.set_candidates(oc["Xc"])
        mu, sd = engine.posterior(0, ym, ys_)
        bi, bv, si, sv, ys = engine.acq_argbest(O.EI, 0.01, oc["y_max"], k_seeds=10, return_values=True)
        return mu, sd, ys, bi, tuple(si)

    on = run()
    t_on = engine.last_timings()
    assert t_on["fit"] > 0 and t_on["posterior_main"] > 0 and t_on["acq_argbest"] > 0
    try:
        engine.set_timing(False)
        assert not engine.timing
        off = run()
        assert all(v == -1.0 for v in engine.last_timings().values())
    finally:
        engine.set_timing(True)
    assert all(np.array_equal(a, b) for a, b in zip(on[:3], off[:3])) and on[3:] == off[3:]
    again = run()
    assert engine.last_timings()["posterior_main"] > 0
    assert all(np.array_equal(a, b) for a, b in zip(on[:3], again[:3]))


def test_virtual_rank_sharding_equals_single_pass(engine):
    """SURVEY.md §8e 'testing without 8 GPUs': G virtual ranks on one device + host merge == one pass."""
    from bayesianoptimization_amd.distributed import merge_best, shard_range

    w = W.P2
    oc = oracle_case(w, 0.6)
    yn, ym, ys_ = O.normalize_targets(oc["y"])
    engine.fit(oc["X"], yn, w.kernel, 0.6, w.noise)
    engine.set_candidates(oc["Xc"])
    engine.posterior(0, ym, ys_, fetch=False)
    full = engine.acq_argbest(w.acq, w.acq_param, oc["y_max"], k_seeds=10)
    for G in (2, 3, 8):
        bv, bi, sv, si = [], [], [], []
        for r in range(G):
            s, e = shard_range(w.M, G, r)
            engine.set_candidates(oc["Xc"][s:e])
            engine.posterior(0, ym, ys_, fetch=False)
            a, b, c, d, _ = engine.acq_argbest(w.acq, w.acq_param, oc["y_max"], k_seeds=10, index_offset=s)
            bi.append(a); bv.append(b); si.append(c); sv.append(d)
        m = merge_best(bv, bi, sv, si, 10)
        assert m[0] == full[0] and m[1] == full[1]
        assert np.array_equal(m[2], full[2]) and np.array_equal(m[3], full[3])


def test_rccl_single_rank_roundtrip(engine):
    """The RCCL transport (dlopen'ed librccl, ncclCommInitRank + ncclAllGather) with world_size = 1."""
    from bayesianoptimization_amd.engine import GpEngine

    uid = GpEngine.comm_unique_id()
    assert len(uid) == 128
    engine.comm_init(uid, 1, 0)
    try:
        vals = np.array([0.5, -1.25, np.nan, 3.0])
        idxs = np.array([7, 1 << 40, 3, -1], dtype=np.int64)
        av, ai = engine.comm_allgather_best(vals, idxs)
        assert np.array_equal(av, vals, equal_nan=True) and np.array_equal(ai, idxs)
    finally:
        engine._lib.gpbo_comm_destroy(engine._h)
        engine.world_size, engine.rank = 1, 0


def test_rccl_local_failure_enters_the_exchange_and_surfaces_as_an_error(debug_engine):
    """A rank whose local acquisition pass failed (here: injected through the debug build's gpbo_debug_fail_next_acq) still
    enters ncclAllGather with a poisoned record, so the collective completes on every rank and the call returns an error
    instead of leaving its peers blocked; the communicator stays usable for the next step."""
    from bayesianoptimization_amd.engine import GpEngine

    engine = debug_engine

    X, y = _data(120, 3, seed=5)
    yn, ym, ys = O.normalize_targets(y)
    engine.fit(X, yn, O.MATERN25, 0.6, 1e-6)
    engine.set_candidates(np.random.RandomState(6).uniform(size=(1000, 3)))
    engine.posterior(0, ym, ys, fetch=False)
    engine.comm_init(GpEngine.comm_unique_id(), 1, 0)
    try:
        good = engine.comm_acq_argbest(O.UCB, 2.0, k_seeds=4)
        assert good[:2] == engine.acq_argbest(O.UCB, 2.0, k_seeds=4)[:2]
        engine.debug_fail_next_acq()
        with pytest.raises(_lib.GpboError, match="injected local failure"):
            engine.comm_acq_argbest(O.UCB, 2.0, k_seeds=4)
        again = engine.comm_acq_argbest(O.UCB, 2.0, k_seeds=4)
        assert again[:2] == good[:2] and np.array_equal(again[2], good[2])
    finally:
        engine._lib.gpbo_comm_destroy(engine._h)
        engine.world_size, engine.rank = 1, 0


@pytest.mark.parametrize("N,d,kernel,ls", [
    (60, 3, O.MATERN25, 0.7), (200, 5, O.RBF, 0.6), (130, 4, O.MATERN25, [0.4, 0.7, 1.0, 1.3]),
    (257, 8, O.RBF, [0.8] * 8), (1, 2, O.MATERN25, 1.0), (700, 16, O.MATERN25, 1.5),
    (2048, 16, O.MATERN25, 1.5), (4096, 16, O.MATERN25, 1.5),      # NP >= 2048: the per-lane-stream path of gpbo_lml_batch
])
def test_lml_value_and_gradient_parity(engine, N, d, kernel, ls):
    """gpbo_lml vs sklearn's log_marginal_likelihood(theta, eval_gradient=True) (_gpr.py:575-652) via the
    oracle restatement: value 1e-10, gradient 1e-7 relative to its largest component."""
    X, y = _data(N, d, seed=11)
    yn, _, _ = O.normalize_targets(y)
    lml_o, grad_o = O.log_marginal_likelihood(kernel, X, yn, ls, 1e-6)
    lml, grad = engine.lml(X, yn, kernel, ls, 1e-6)
    assert abs(lml - lml_o) <= 1e-10 * max(1.0, abs(lml_o))
    assert np.max(np.abs(grad - grad_o)) <= 1e-7 * max(np.max(np.abs(grad_o)), 1e-12)
    assert engine.lml(X, yn, kernel, ls, 1e-6, eval_gradient=False) == lml
    if N >= 2048:     # two lanes on their own streams: each bitwise the single evaluation
        ls2 = np.array([[float(np.atleast_1d(ls)[0])], [0.9]])
        (v0, g0), (v1, g1) = engine.lml_batch(X, yn, kernel, ls2, 1e-6)
        assert v0 == lml and np.array_equal(g0, grad)
        v1s, g1s = engine.lml(X, yn, kernel, 0.9, 1e-6)
        assert v1 == v1s and np.array_equal(g1, g1s)
    with pytest.raises(_lib.GpboError):
        engine.posterior(0)   # gpbo_lml leaves the slot unfitted


def test_lml_not_pd_returns_minus_inf(engine):
    X = np.array([[0.1, 0.2], [0.1, 0.2], [0.5, 0.5]])
    lml, grad = engine.lml(X, np.zeros(3), O.RBF, 1.0, 0.0)
    assert lml == -np.inf and np.all(grad == 0)


@pytest.mark.parametrize("M", [1, 2, 3, 5, 8, 17, 170])
@pytest.mark.parametrize("N,d,kernel,ls", [(150, 6, O.MATERN25, 0.8), (1030, 16, O.MATERN25, 1.5), (70, 2, O.RBF, 0.5)])
def test_small_batch_path_equals_oracle_and_big_kernel(debug_engine, M, N, d, kernel, ls):
    """M <= 8 goes through the batched-GEMV latency path (posterior_small.hip): same results as the oracle
    and as the MFMA kernel (GPBO_POST_SMALL=0, a debug-build switch) to rounding."""
    import os

    engine = debug_engine

    X, y = _data(N, d, seed=21)
    gp = O.fit_fixed_theta(kernel, X, y, ls, 1e-6)
    yn, ym, ys = O.normalize_targets(y)
    engine.fit(X, yn, kernel, ls, 1e-6)
    Xc = np.random.RandomState(22).uniform(size=(M, d))
    Xc[0] = X[3]                                   # a training point: variance ~ alpha, the cancellation case
    mu, sd = engine.predict(Xc, y_mean=ym, y_std=ys)
    mu_o, sd_o = O.predict(gp, Xc)
    tol = 1e-7 if kernel == O.RBF else 1e-9
    assert np.max(np.abs(mu - mu_o)) <= tol * np.max(np.abs(mu_o))
    assert np.max(np.abs(sd - sd_o)) <= tol * max(np.max(np.abs(sd_o)), 1e-3)
    os.environ["GPBO_POST_SMALL"] = "0"
    try:
        mu_b, sd_b = engine.predict(Xc, y_mean=ym, y_std=ys)
    finally:
        os.environ.pop("GPBO_POST_SMALL")
    # the two device paths sum k*.alpha and |W k*|^2 in different orders: agreement is bounded by the same
    # kappa(K)*eps noise as the comparison with LAPACK (RBF, N=70, d=2: kappa ~ 4e7, |alpha| ~ 1e5)
    assert np.max(np.abs(mu - mu_b)) <= tol * np.max(np.abs(mu_o))
    assert np.max(np.abs(sd - sd_b)) <= tol * max(np.max(np.abs(sd_o)), 1e-3)


@pytest.mark.parametrize("M", [9, 1000, 1024, 10000, 20001])
@pytest.mark.parametrize("N,d,kernel,ls", [(25, 2, O.MATERN25, 2.2), (64, 3, O.RBF, 0.3), (200, 6, O.MATERN25, 0.8), (256, 17, O.MATERN25, 1.1),
                                              (270, 5, O.MATERN25, 0.7), (400, 5, O.RBF, 0.4), (512, 8, O.MATERN25, [0.6 + 0.1 * t for t in range(8)])])
def test_posterior_with_both_ends_in_the_launch_is_bitwise_the_three_launches(debug_engine, N, d, kernel, ls, M):
    """Round 6: when one workgroup of the fused posterior kernel holds every row of its candidates (NP <= 256 on the 8-wave kernel,
    384 <= NP <= 512 on the 16-wave one) the launch takes the RAW candidates (scaled on their way into LDS) and writes mu and sd
    itself — prescale_kernel and posterior_finalize_kernel are gone from the pass, 3 launches -> 1.  Same arithmetic element for
    element (prescale_elem's division, posterior_finalize_elem): bitwise the three launches (GPBO_POST_FUSE_ENDS=0, debug build),
    ragged candidate counts, a candidate ON a training point (variance clipped at 0: the flag) and per-dimension length scales
    included.  M = 9 with GPBO_POST_SMALL=0 keeps the MFMA kernel on a batch the latency path would take."""
    import os

    engine = debug_engine
    X, y = _data(N, d, seed=71)
    yn, ym, ys = O.normalize_targets(y)
    engine.fit(X, yn, kernel, ls, 1e-10)
    Xc = np.random.RandomState(72).uniform(size=(M, d))
    Xc[min(7, M - 1)] = X[3]
    os.environ["GPBO_POST_SMALL"] = "0"
    try:
        engine.take_negative_variance_flag()
        mu, sd = engine.predict(Xc, y_mean=ym, y_std=ys)
        flag = engine.take_negative_variance_flag()
        os.environ["GPBO_POST_FUSE_ENDS"] = "0"
        mu3, sd3 = engine.predict(Xc, y_mean=ym, y_std=ys)
        flag3 = engine.take_negative_variance_flag()
    finally:
        os.environ.pop("GPBO_POST_SMALL")
        os.environ.pop("GPBO_POST_FUSE_ENDS", None)
    assert np.array_equal(mu, mu3) and np.array_equal(sd, sd3) and flag == flag3
    gp = O.fit_fixed_theta(kernel, X, y, ls, 1e-10)
    mu_o, sd_o = O.predict(gp, Xc)
    assert np.max(np.abs(mu - mu_o)) <= 1e-6 * np.max(np.abs(mu_o))


@pytest.mark.parametrize("N,d,kernel,ls", [(270, 5, O.MATERN25, 0.7), (400, 6, O.MATERN25, 0.9), (512, 8, O.MATERN25, 1.0), (700, 3, O.RBF, 0.25),
                                              (1000, 17, O.MATERN25, [0.7 + 0.05 * t for t in range(17)]), (1024, 33, O.RBF, 1.4)])
def test_the_three_large_batch_posterior_kernels_agree(debug_engine, N, d, kernel, ls):
    """For 384 <= NP <= 512 and a batch that fills the chip the posterior runs on the fused 16-wave kernel with 512-row
    chunks ("v4", round 4: k* generated once per candidate tile, never through HBM; instantiated up to NP = 1024); the
    fused 256-row-chunk kernel (v2) and the k* slab + GEMM pipeline (v3) compute the same quantities from the same packed
    W.  The debug build's GPBO_POST_KERNEL forces each in turn: all three agree with each other to summation order (1e-12; RBF: 1e-9)
    and with the oracle (1e-9; 1e-8 for the RBF cases, kappa(K) ~ 1e8: two CPU algorithms differ by as much there) on every
    candidate, ragged last chunk (N = 400, 700), a ragged candidate tile and per-dimension length scales included — what
    sklearn's predict(return_std=True) gives (_gpr.py:443-494)."""
    import os

    engine = debug_engine
    X, y = _data(N, d, seed=61)
    gp = O.fit_fixed_theta(kernel, X, y, ls, 1e-6)
    yn, ym, ys = O.normalize_targets(y)
    engine.fit(X, yn, kernel, ls, 1e-6)
    Xc = np.random.RandomState(62).uniform(size=(17001, d))
    Xc[7] = X[3]
    engine.set_candidates(Xc)
    out = {}
    for path in ("4", "3", "2", None):
        if path is None:
            os.environ.pop("GPBO_POST_KERNEL", None)
        else:
            os.environ["GPBO_POST_KERNEL"] = path
        try:
            out[path] = engine.posterior(0, ym, ys)
        finally:
            os.environ.pop("GPBO_POST_KERNEL", None)
    mu_o, sd_o = O.predict(gp, Xc)
    tol = 1e-8 if kernel == O.RBF else 1e-9
    for path, (mu, sd) in out.items():
        assert rel_err(mu, mu_o) <= tol and rel_err(sd, sd_o) <= tol, path
    xtol = 1e-9 if kernel == O.RBF else 1e-12      # (RBF, kappa ~ 1e8: |alpha| ~ 1e5, so the order of the k*.alpha sum shows at 1e-10)
    for path in ("3", "2"):
        assert rel_err(out[path][0], out["4"][0]) <= xtol and rel_err(out[path][1], out["4"][1]) <= 10 * xtol, path
    # the default dispatch for a batch of this size (17 001 candidates: between the 16-wave kernel's one-round range, <= 16 384, and 32 768)
    want = "2" if 256 < (N + 63) // 64 * 64 <= 512 else "3"
    assert np.array_equal(out[None][0], out[want][0]) and np.array_equal(out[None][1], out[want][1])


def test_small_batch_rows_do_not_depend_on_the_batch(debug_engine):
    """The GEMV path evaluates every candidate with the same instruction sequence whatever batch it arrives in
    (pass width 1/2/4/8/16, pass index): a lockstep round of n_seeds * (d + 1) points returns, row for row, the
    bits the per-run batches of d + 1 points return — what lets the merged L-BFGS-B runs retrace the separate ones.
    (GPBO_SMALL_MAX pins the path: a debug-build switch.)"""
    import os

    engine = debug_engine

    N, d = 700, 9
    X, y = _data(N, d, seed=51)
    yn, ym, ys = O.normalize_targets(y)
    engine.fit(X, yn, O.MATERN25, 1.1, 1e-6)
    Xc = np.random.RandomState(52).uniform(size=(10 * (d + 1) + 3, d))
    os.environ["GPBO_SMALL_MAX"] = "1024"
    try:
        mu_all, sd_all = engine.predict(Xc, y_mean=ym, y_std=ys)
        for lo, hi in [(0, 1), (1, 3), (3, 13), (13, 30), (30, 103), (100, 103)]:
            mu, sd = engine.predict(Xc[lo:hi], y_mean=ym, y_std=ys)
            assert np.array_equal(mu, mu_all[lo:hi]) and np.array_equal(sd, sd_all[lo:hi])
    finally:
        os.environ.pop("GPBO_SMALL_MAX")


# The slab paths (posterior_plan.h): how each is reached, its padded size NP (each with a ragged last row chunk for its own GEMM)
# and the bytes of one k* value in its slab.
_SLAB_PATHS = {
    "f64": dict(NP=640, elem=8, f32=False, debug=False),       # SlabF64, 256-row chunks
    "f32_16": dict(NP=320, elem=4, f32=True, debug=False),     # SlabF32 on 16x16 MFMAs, 256-row chunks
    "f32_32": dict(NP=576, elem=4, f32=True, debug=False),     # SlabF32 on 32x32 MFMAs, 512-row chunks
    "i8": dict(NP=576, elem=7, f32=False, debug=True),         # SlabI8 (GPBO_POST_KERNEL=8: debug build), 128-row chunks
}
_slab_oracles = {}


def _slab_case(N, d, kernel):
    """Inputs and the oracle's posterior for one (N, d, kernel), computed once and shared by the paths that use it."""
    key = (N, d, kernel)
    if key not in _slab_oracles:
        X, y = _data(N, d, seed=41)
        Xc = np.random.RandomState(42).uniform(size=(1000, d))      # Mp = 1024
        Xc[7] = X[3]                                                 # a training point: variance ~ noise, the cancellation case
        mu_o, sd_o = O.predict(O.fit_fixed_theta(kernel, X, y, 0.9, 1e-6), Xc)
        for a in (X, y, Xc, mu_o, sd_o):
            a.setflags(write=False)
        _slab_oracles[key] = (X, y, Xc, mu_o, sd_o)
    return _slab_oracles[key]


@pytest.mark.parametrize("d,kernel", [(5, O.MATERN25), (17, O.MATERN25), (17, O.RBF)])       # DP = 8, 32
@pytest.mark.parametrize("path", list(_SLAB_PATHS))
def test_kstar_slab_loop_equals_single_slab(request, path, d, kernel):
    """The k* slab is bounded by a workspace budget; a candidate set larger than one slab is walked slab by slab (one walk and
    one k* generator for the three slab paths: launch_posterior_slabs, kstar_gen_kernel).  Per path, with padded train rows
    (N = NP - 2) and 1000 candidates (Mp = 1024): the pass over ONE slab, over slabs of 384 candidates (384 + 384 + 256: a
    narrower last slab) and over eight slabs of 128 (half of every generator workgroup idle) — widths forced through
    GPBO_KSTAR_GB from the path's bytes per candidate — give bitwise the same mu and sd, and the single-slab pass agrees with
    the oracle at its path's bar: TOL in fp64, test_gpu_f32.py's in fp32, test_gpu_int8_posterior.py's elementwise 1e-5 on the
    int8 GEMM."""
    import os

    from bayesianoptimization_amd.engine import F32, F64

    row = _SLAB_PATHS[path]
    engine = request.getfixturevalue("debug_engine" if row["debug"] else "engine")
    NP = row["NP"]
    X, y, Xc, mu_o, sd_o = _slab_case(NP - 2, d, kernel)
    yn, ym, ys = O.normalize_targets(y)
    engine.fit(X, yn, kernel, 0.9, 1e-6, precision=F32 if row["f32"] else F64)
    engine.set_candidates(Xc)
    if row["debug"]:
        os.environ["GPBO_POST_KERNEL"] = "8"
    out = {}
    try:
        for width in (None, 384, 128):
            if width is not None:
                os.environ["GPBO_KSTAR_GB"] = repr(width * NP * row["elem"] / 1e9 * 1.01)    # room for `width` candidates per slab
            out[width] = engine.posterior(0, ym, ys)
    finally:
        os.environ.pop("GPBO_KSTAR_GB", None)
        os.environ.pop("GPBO_POST_KERNEL", None)
    mu, sd = out[None]
    for width in (384, 128):
        assert np.array_equal(mu, out[width][0]) and np.array_equal(sd, out[width][1]), width
    if path == "f64":
        errs = (rel_err(mu, mu_o), rel_err(sd, sd_o))
        print(path, d, kernel, "rel_err mu, sd:", errs)
        assert errs[0] < TOL and errs[1] < TOL
    elif row["f32"]:
        errs = (rel_err(mu, mu_o), float(np.max(np.abs(sd**2 - sd_o**2)) / ys**2))
        print(path, d, kernel, "rel_err mu, max |sd^2 - sd_o^2| / ys^2:", errs)
        assert errs[0] < 1e-7 and errs[1] < 2e-5
    else:
        pos = sd_o > 0
        errs = (float(np.max(np.abs(mu - mu_o) / np.maximum(np.abs(mu_o), ys))), float(np.max(np.abs(sd - sd_o)[pos] / sd_o[pos])))
        print(path, d, kernel, "elementwise mu, sd:", errs)
        assert errs[0] <= 1e-5 and errs[1] <= 1e-5


# ---- gpbo_fit_append ---------------------------------------------------------------------
@pytest.mark.parametrize("kernel,ls", [(O.MATERN25, 0.9), (O.RBF, 1.3)])
@pytest.mark.parametrize("n0,steps", [(100, [1, 3, 1]), (126, [1, 1, 5]), (128, [1]), (60, [20]), (200, [0, 2, 0])])
def test_fit_append_equals_full_fit(engine, kernel, ls, n0, steps):
    """Rows appended one call at a time (inside the 64-row padding: rank-one growth; across it, n_new > 16 or
    n_new = 0: the other branches) give the model a from-scratch fit of all rows gives; the appended K row is bitwise
    the full fit's."""
    d = 5
    X, y = _data(n0 + sum(steps), d, seed=61)
    Xc = np.random.RandomState(62).uniform(size=(300, d))
    n = n0
    yn, ym, ys = O.normalize_targets(y[:n])
    engine.fit(X[:n], yn, kernel, ls, 1e-6)
    for k in steps:
        n += k
        yn, ym, ys = O.normalize_targets(y[:n] if k else 2.0 * y[:n] + 1.0)
        engine.fit_append(X[n - k:n], yn)
        # RBF at this length scale: cond(K) ~ 1e8, the usual kappa * eps allowance (see test_small_batch_path_*)
        _assert_same_model(engine, X[:n], yn, kernel, ls, 1e-6, ym, ys, Xc, tol=1e-9 if kernel == O.MATERN25 else 1e-6)
    K_inc = engine.get_K(n)
    engine.fit(X[:n], yn, kernel, ls, 1e-6)
    assert np.array_equal(K_inc, engine.get_K(n))


def test_fit_append_f32_mode_and_errors(engine):
    from bayesianoptimization_amd.engine import F32

    d = 4
    X, y = _data(150, d, seed=63)
    yn, ym, ys = O.normalize_targets(y[:140])
    engine.fit(X[:140], yn, O.MATERN25, 0.8, 1e-6, precision=F32)
    yn, ym, ys = O.normalize_targets(y[:143])
    engine.fit_append(X[140:143], yn)
    Xc = np.random.RandomState(64).uniform(size=(500, d))
    mu, sd = engine.predict(Xc, y_mean=ym, y_std=ys)
    gp = O.fit_fixed_theta(O.MATERN25, X[:143], yn, 0.8, 1e-6, normalize_y=False)
    mu_o, sd_o = O.predict(gp, Xc)
    assert rel_err(mu, ys * mu_o + ym) < 1e-5
    assert np.max(np.abs(sd**2 - (ys * sd_o) ** 2)) <= 2e-5 * ys**2
    with pytest.raises(ValueError):
        engine.fit_append(X[143:145], yn)                      # n_total != N + n_new
    with pytest.raises(ValueError):
        engine.fit_append(np.zeros((1, d + 1)), np.zeros(144))   # wrong d
    # a new pivot that is not > 0 (here: NaN from a NaN input, the deterministic way to get one) -> LinAlgError
    # naming the order of the failing minor, slot left unfitted
    engine.fit(X[:50], O.normalize_targets(y[:50])[0], O.RBF, 1.0, 1e-6)
    with pytest.raises(np.linalg.LinAlgError, match="51"):
        engine.fit_append(np.full((1, d), np.nan), np.zeros(51))
    with pytest.raises(_lib.GpboError):
        engine.posterior(0)
    with pytest.raises(_lib.GpboError):
        engine.fit_append(X[50:51], np.zeros(51))              # nothing fitted to append to
    engine.lml(X[:50], np.zeros(50), O.RBF, 1.0, 1e-6)
    with pytest.raises(_lib.GpboError):
        engine.fit_append(X[50:51], np.zeros(51))              # gpbo_lml clobbered the slot


def test_fit_append_long_run_stays_accurate():
    """300 consecutive single-row appends (crossing the padding several times, i.e. mixing rank-one growth with
    rebuilds and, on this FRESH context whose slot starts at 256 rows of capacity, reallocations) do not drift: the
    final model is the from-scratch model to the usual tolerance."""
    from bayesianoptimization_amd.engine import GpEngine

    engine = GpEngine(0)
    d = 6
    X, y = _data(500, d, seed=65)
    n = 200
    engine.fit(X[:n], O.normalize_targets(y[:n])[0], O.MATERN25, 1.1, 1e-6)
    for n in range(201, 501):
        yn, ym, ys = O.normalize_targets(y[:n])
        engine.fit_append(X[n - 1:n], yn)
    _assert_same_model(engine, X[:500], yn, O.MATERN25, 1.1, 1e-6, ym, ys, np.random.RandomState(66).uniform(size=(64, d)))
    engine.close()


@pytest.mark.parametrize("N,d,kernel", [(300, 4, O.MATERN25), (1030, 9, O.RBF)])
def test_lml_batch_lanes_are_bitwise_gpbo_lml(engine, N, d, kernel):
    """gpbo_lml_batch: every lane (its own K, L, W in the shared slab) returns the bits gpbo_lml returns for that theta;
    anisotropic rows too; a non-PD lane reports -inf without disturbing its neighbours; the model slots keep their fits."""
    X, y = _data(N, d, seed=71)
    yn, ym, ys = O.normalize_targets(y)
    engine.fit(X, yn, kernel, 1.0, 1e-6)
    Xc = np.random.RandomState(72).uniform(size=(200, d))
    before = engine.predict(Xc, y_mean=ym, y_std=ys)
    scales = np.array([[0.3], [0.7], [1.0], [1.9], [4.0], [0.05], [11.0], [0.5]])
    got = engine.lml_batch(X, yn, kernel, scales, 1e-6)
    after = engine.predict(Xc, y_mean=ym, y_std=ys)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    for (val, grad), ls in zip(got, scales):
        v1, g1 = engine.lml(X, yn, kernel, ls, 1e-6)
        assert val == v1 and np.array_equal(grad, g1)
        if 0.2 <= ls[0] <= 2.0:     # the well-conditioned thetas also against the oracle (the others: cond(K) >> 1e10)
            v_o, g_o = O.log_marginal_likelihood(kernel, X, yn, ls, 1e-6, True)
            assert abs(val - v_o) <= (1e-9 if kernel == O.MATERN25 else 1e-6) * abs(v_o)
    # the same shape again: the second call captures each lane's launch sequence into a hipGraph, later calls replay
    # it — new thetas enter through the pinned length-scale words; still bitwise gpbo_lml, for fewer lanes too
    for rep in range(4):
        sc = np.random.RandomState(80 + rep).uniform(0.3, 3.0, size=(8 if rep < 3 else 5, 1))
        for (val, grad), ls in zip(engine.lml_batch(X, yn, kernel, sc, 1e-6), sc):
            v1, g1 = engine.lml(X, yn, kernel, ls, 1e-6)
            assert val == v1 and np.array_equal(grad, g1)
    vals_only = engine.lml_batch(X, yn, kernel, scales[:3], 1e-6, eval_gradient=False)
    assert [v for v, _ in vals_only] == [v for v, _ in got[:3]]
    aniso = np.random.RandomState(73).uniform(0.4, 2.0, size=(3, d))
    for (val, grad), ls in zip(engine.lml_batch(X, yn, kernel, aniso, 1e-6), aniso):
        v1, g1 = engine.lml(X, yn, kernel, ls, 1e-6)
        assert val == v1 and np.array_equal(grad, g1) and grad.shape == (d,)
    Xdup = X.copy()
    Xdup[1] = Xdup[0]
    mixed = engine.lml_batch(Xdup, yn, O.RBF, np.array([[1.0], [0.8]]), 0.0)
    assert all(v == -np.inf and np.all(g == 0) for v, g in mixed)
    with pytest.raises(ValueError):
        engine.lml_batch(X, yn, kernel, np.ones((9, 1)), 1e-6)


@pytest.mark.parametrize("N,d", [(2100, 5), (4096, 16)])
def test_lml_lanes_dealt_to_two_groups_are_bitwise_gpbo_lml(engine, N, d):
    """Round 6: from NP = 2048 on the lanes of a gpbo_lml_batch call are dealt to TWO groups (two streams is what the hardware
    queues run side by side; inside a group lane = a grid dimension, so the diagonal blocks of its lanes factor in one launch) —
    (n + 1) / 2 lanes per group below NP = 4096, two per group above for n >= 4.  Whatever the dealing, every lane returns the bits
    gpbo_lml returns alone; the lane counts below are a theta search's (6, 6, 6, 5, 3, 2, 1, ...) and come round again, so every
    grouping is run directly, captured and replayed from the graph pool."""
    X, y = _data(N, d, seed=91)
    yn, _, _ = O.normalize_targets(y)
    rng = np.random.RandomState(92)
    single = {}

    def alone(ls):
        key = float(ls)
        if key not in single:
            single[key] = engine.lml(X, yn, O.MATERN25, ls, 1e-6)
        return single[key]

    pool = rng.uniform(0.6, 2.5, size=8).round(3)
    for n in (6, 6, 6, 5, 3, 2, 1, 1, 4, 6, 5, 3, 2, 4, 6):
        sc = rng.choice(pool, size=(n, 1), replace=False)
        for (val, grad), ls in zip(engine.lml_batch(X, yn, O.MATERN25, sc, 1e-6), sc):
            v1, g1 = alone(ls[0])
            assert np.isfinite(val) and val == v1 and np.array_equal(grad, g1)


@pytest.mark.parametrize("N,d,kernel,ls,M", [(60, 3, O.MATERN25, 0.7, 1), (200, 5, O.RBF, 0.6, 7), (513, 8, O.MATERN25, 1.0, 10),
                                             (130, 4, O.MATERN25, [0.4, 0.7, 1.0, 1.3], 33), (1000, 16, O.MATERN25, 1.5, 64),
                                             (300, 40, O.RBF, 2.5, 256)])
def test_predict_grad_equals_the_oracle_gradient(engine, N, d, kernel, ls, M):
    """gpbo_predict_grad: mu, sd bitwise-or-rounding the small-batch predict, d mu / d x and d sd / d x
    against the oracle's analytic gradient (itself pinned to central differences on CPU)."""
    X, y = _data(N, d)
    gp = O.fit_fixed_theta(kernel, X, y, ls, 1e-6)
    yn, ym, ys_ = O.normalize_targets(y)
    engine.fit(X, yn, kernel, ls, 1e-6)
    Xq = np.random.RandomState(5).uniform(size=(M, d))
    mu, sd, dmu, dsd = engine.predict_grad(Xq, 0, ym, ys_)
    mu_o, sd_o, dmu_o, dsd_o = O.predict_grad(gp, Xq)
    assert rel_err(mu, mu_o) < 1e-8 and rel_err(sd, sd_o) < 1e-7
    assert rel_err(dmu, dmu_o) < 1e-7 and rel_err(dsd, dsd_o) < 1e-6
    # a training point: the clipped variance has zero slope, nothing is NaN
    mu1, sd1, dmu1, dsd1 = engine.predict_grad(X[:3], 0, ym, ys_)
    assert np.all(np.isfinite(dmu1)) and np.all(np.isfinite(dsd1))


@pytest.mark.parametrize("N,d,kernel,ls,M", [(60, 3, O.MATERN25, 0.7, 5), (200, 5, O.RBF, 0.6, 130), (513, 8, O.MATERN25, 1.0, 300),
                                             (1100, 16, O.MATERN25, 1.5, 257)])
def test_predict_cov_equals_sklearn_return_cov(engine, N, d, kernel, ls, M):
    """gpbo_predict_cov against GaussianProcessRegressor.predict(return_cov=True) (_gpr.py:458-469), and
    HipGPR.predict(return_cov=True) — the call BayesianOptimization.predict(return_cov=True) makes."""
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, Matern

    from bayesianoptimization_amd.gpr import HipGPR

    X, y = _data(N, d)
    k = Matern(nu=2.5, length_scale=ls) if kernel == O.MATERN25 else RBF(length_scale=ls)
    sk = GaussianProcessRegressor(kernel=k, alpha=1e-6, normalize_y=True, optimizer=None).fit(X, y)
    Xq = np.random.RandomState(6).uniform(size=(M, d))
    mu_s, cov_s = sk.predict(Xq, return_cov=True)
    gp = HipGPR(kernel=k, alpha=1e-6, normalize_y=True, optimizer=None, engine=engine).fit(X, y)
    mu, cov = gp.predict(Xq, return_cov=True)
    assert cov.shape == (M, M)
    assert rel_err(mu, mu_s) < 1e-8
    assert np.max(np.abs(cov - cov_s)) < 1e-8 * np.max(np.abs(cov_s))
    assert np.max(np.abs(cov - cov.T)) < 1e-12 * np.max(np.abs(cov_s))
    _, sd = gp.predict(Xq, return_std=True)
    assert np.max(np.abs(np.sqrt(np.clip(np.diag(cov), 0, None)) - sd)) < 1e-6 * np.max(sd)


def test_overlapped_fits_are_bitwise_the_sequential_fits(engine):
    """gpbo_fit_begin / gpbo_fit_wait (GpEngine.overlapped_fits): the target GP and the constraint GPs of one suggest()
    (acquisition.py:84-86) factorised side by side on their slots' own streams.  Every slot must hold bitwise what gpbo_fit
    gives it; a read inside the block waits for that slot only; a non-PD matrix raises when the block ends while the other
    slots' fits stand; misuse of the two entry points is reported."""
    import ctypes as C

    from bayesianoptimization_amd import _lib
    from bayesianoptimization_amd.engine import F32, F64

    N, d = 1500, 6
    X, y = _data(N, d)
    y2 = np.cos(2.0 * X.sum(axis=1))
    y3 = X[:, 0] - X[:, 1] ** 2
    jobs = [(0, y, O.MATERN25, 0.9, F64), (1, y2, O.RBF, 0.7, F64), (2, y3, O.MATERN25, 1.3, F32)]

    def norm(v):
        return (v - v.mean()) / v.std()

    ref = {}
    for slot, yy, kern, ls, prec in jobs:
        engine.fit(X, norm(yy), kern, ls, 1e-6, slot=slot, precision=prec)
        ref[slot] = (engine.get_L(N, slot), engine.get_Linv(N, slot), engine.get_alpha(N, slot))
    Xq = np.random.RandomState(3).uniform(size=(3000, d))
    post_ref = {slot: engine.predict(Xq, slot) for slot, *_ in jobs}

    with engine.overlapped_fits():
        for slot, yy, kern, ls, prec in jobs:
            engine.fit(X, norm(yy), kern, ls, 1e-6, slot=slot, precision=prec)
        assert engine._pending_fits == {0, 1, 2}
        mu1, sd1 = engine.predict(Xq, 1)                    # reads slot 1: waits for slot 1 only
        assert engine._pending_fits == {0, 2}
        assert np.array_equal(mu1, post_ref[1][0]) and np.array_equal(sd1, post_ref[1][1])
    assert not engine._pending_fits
    for slot, *_ in jobs:
        L, Wm, a = engine.get_L(N, slot), engine.get_Linv(N, slot), engine.get_alpha(N, slot)
        assert np.array_equal(L, ref[slot][0]) and np.array_equal(Wm, ref[slot][1]) and np.array_equal(a, ref[slot][2])
        mu, sd = engine.predict(Xq, slot)
        assert np.array_equal(mu, post_ref[slot][0]) and np.array_equal(sd, post_ref[slot][1])

    # not positive definite: duplicate rows, no noise -> LinAlgError when the block ends; slot 0's fit stands
    Xbad = np.array([[0.1, 0.2], [0.1, 0.2], [0.5, 0.5]])
    with pytest.raises(np.linalg.LinAlgError, match="not returning a positive definite matrix"):
        with engine.overlapped_fits():
            engine.fit(X, norm(y), O.MATERN25, 0.9, 1e-6, slot=0)
            engine.fit(Xbad, np.zeros(3), O.MATERN25, 1.0, 0.0, slot=1)
    assert not engine._pending_fits
    assert np.array_equal(engine.get_L(N, 0), ref[0][0])
    with pytest.raises(Exception):
        engine.posterior(1)                                  # slot 1 is unfitted

    # the C entry points refuse misuse
    lib = _lib.load_library()
    info = C.c_int(0)
    assert lib.gpbo_fit_wait(engine._h, 0, C.byref(info)) == _lib.ERR_STATE
    yn = np.ascontiguousarray(norm(y))
    ls = np.array([0.9])
    Xc_ = np.ascontiguousarray(X)
    assert lib.gpbo_fit_begin(engine._h, 0, _lib.dptr(Xc_), _lib.dptr(yn), N, d, O.MATERN25, _lib.dptr(ls), 1, 1e-6, 0) == _lib.GPBO_OK
    assert lib.gpbo_fit_begin(engine._h, 0, _lib.dptr(Xc_), _lib.dptr(yn), N, d, O.MATERN25, _lib.dptr(ls), 1, 1e-6, 0) == _lib.ERR_STATE
    assert lib.gpbo_fit(engine._h, 0, _lib.dptr(Xc_), _lib.dptr(yn), N, d, O.MATERN25, _lib.dptr(ls), 1, 1e-6, 0, C.byref(info)) == _lib.ERR_STATE
    assert lib.gpbo_fit_wait(engine._h, 0, C.byref(info)) == _lib.GPBO_OK and info.value == 0
    assert np.array_equal(engine.get_L(N, 0), ref[0][0])


@pytest.mark.parametrize("N,d", [(700, 6), (1500, 8), (4096, 16), (8192, 16)])
def test_lml_evaluations_do_not_read_above_the_diagonal_of_W(debug_engine, N, d):
    """Round 6: an LML evaluation no longer zero-fills W before W = L^-1 is built (8 N^2 bytes: 18 us of a 2.85 ms evaluation at
    N = 4096) — every reader of the evaluation cuts its k-range at the operand's diagonal tile, and the one tile a 128-row
    granularity can reach (right of an even diagonal block) is cleared with the diagonal blocks.  Here the rest of W is filled
    with NaNs first (libgpbo_dbg.so, GPBO_POISON_W): value and gradient, single and in lanes, stay bitwise what they are without."""
    import os

    X, y = _data(N, d, seed=5)
    yn, _, _ = O.normalize_targets(y)
    scales = np.array([[0.8], [1.3], [2.0]])
    want1 = debug_engine.lml(X, yn, O.MATERN25, 1.3, 1e-6)
    want = debug_engine.lml_batch(X, yn, O.MATERN25, scales, 1e-6)
    os.environ["GPBO_POISON_W"] = "1"           # (the second call of a shape is the one that captures the lanes' graph: poison included)
    try:
        got1 = debug_engine.lml(X, yn, O.MATERN25, 1.3, 1e-6)
        got = debug_engine.lml_batch(X, yn, O.MATERN25, scales, 1e-6)
    finally:
        os.environ.pop("GPBO_POISON_W")
    assert np.isfinite(got1[0]) and got1[0] == want1[0] and np.array_equal(got1[1], want1[1])
    for (v, g), (v0, g0) in zip(got, want):
        assert v == v0 and np.array_equal(g, g0)
    assert want[1][0] == want1[0]
