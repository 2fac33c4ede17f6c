"""CPU: suggest_batch's host logic over an oracle-backed engine double — the picks against tests/batch_truth.py (a from-scratch
refit per pick at held theta and held normalisation), the first pick and the RandomState against one suggest(n_smart=0) of a
twin, the state left behind, the policy's bookkeeping, every refusal, and the engine calls a batch makes (one full posterior,
q - 1 refreshes).  The double's posterior_refresh IS the full posterior: what is checked here is the protocol around it; the
incremental update itself is checked on the device (tests/test_gpu_posterior_refresh.py)."""
import numpy as np
import pytest

import batch_truth as B
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import suggest_batch
from helpers import FakeEngine
from oracle import gp_oracle as O
from oracle.refenv import have_reference, import_reference

D, N, M = 3, 30, 1500          # M * D >= 4096: the candidates are drawn on the engine from the optimizer's RandomState
BOUNDS = B.SUGGEST_BOUNDS


class RefreshFakeEngine(FakeEngine):
    """FakeEngine + posterior_refresh = the full posterior of the slot's (grown) model."""

    def posterior_refresh(self, slot=0, y_mean=0.0, y_std=1.0, fetch=True, return_route=False):
        self.calls.append(("posterior_refresh", slot))
        mu, sd = O.predict(self.models[slot], self.Xc)
        mu, sd = y_std * mu + y_mean, sd * y_std
        self.post[slot] = (mu, sd)
        out = (mu, sd) if fetch else (None, None)
        return (*out, 1) if return_route else out


def _policy(name, **kw):
    return {"ucb": lambda: A.UpperConfidenceBound(kappa=2.0, **kw), "ei": lambda: A.ExpectedImprovement(xi=0.01, **kw),
            "poi": lambda: A.ProbabilityOfImprovement(xi=0.5, **kw)}[name]()


def _driver(policy, seed=3, **kw):
    return B.suggest_driver(RefreshFakeEngine, policy, seed=seed, n_random=M, **kw)


def _theta(gp):
    return int(gp._kind), np.array(gp._ls, dtype=np.float64), float(gp.alpha)


#: RandomState seed per policy, picked on the CPU so that the truth's own gap holds in every case (POI with the 'min' lie saturates
#: near 1 at the third pick under seeds 3 and 5: two candidates 1e-10 apart)
SEEDS = {"ucb": 3, "ei": 3, "poi": 4}


@pytest.mark.parametrize("strategy", ["max", "min", "mean", 0.25])
@pytest.mark.parametrize("name", ["ucb", "ei", "poi"])
def test_picks_equal_the_refit_truth(name, strategy):
    q = 3
    drv, eng, X, y = _driver(_policy(name), seed=SEEDS[name])
    picks = suggest_batch(drv, q, strategy=strategy)
    assert len(picks) == q and all(list(p) == drv._space.keys for p in picks)
    Xc = eng.Xc
    assert Xc.shape == (M, D)
    kind, ls, noise = _theta(drv._gp)
    fn = drv._acquisition_function
    params = [fn._acq_param()] * q           # no decay configured
    want, gaps = B.batch_truth(kind, ls, noise, X, y, Xc, fn._acq_kind, params, strategy, q)
    assert gaps.min() >= B.GAP_FLOOR, f"the truth's own best / second gap {gaps.min():.2e}: pick another seed"
    assert np.array_equal(B.rows_to_indices(picks, Xc), want)
    assert len(set(want.tolist())) == q      # the lie moves the next pick off the previous one


@pytest.mark.parametrize("name", ["ucb", "ei"])
def test_one_pick_is_the_twins_suggest_and_leaves_its_randomstate(name):
    drv, eng, _, _ = _driver(_policy(name))
    twin, teng, _, _ = _driver(_policy(name))
    x_twin = twin.suggest_first()
    (pick,) = suggest_batch(drv, 1)
    assert np.array_equal(np.array(list(pick.values())), x_twin)
    # a longer batch starts with the same pick and draws nothing more
    drv3, _, _, _ = _driver(_policy(name))
    picks = suggest_batch(drv3, 4)
    assert np.array_equal(np.array(list(picks[0].values())), x_twin)
    for d_ in (drv, drv3):
        a, b = d_._random_state.get_state(), twin._random_state.get_state()
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_predict_answers_for_the_real_data_afterwards():
    drv, eng, X, y = _driver(_policy("ucb"), n_restarts_optimizer=0)      # no restarts: the theta search draws nothing
    drv.suggest_first()
    Xq = BOUNDS[:, 0] + np.random.RandomState(9).uniform(size=(40, D)) * (BOUNDS[:, 1] - BOUNDS[:, 0])
    mu0, sd0 = drv._gp.predict(Xq, return_std=True)
    suggest_batch(drv, 5, strategy="max")
    mu1, sd1 = drv._gp.predict(Xq, return_std=True)
    assert np.array_equal(mu0, mu1) and np.array_equal(sd0, sd1)
    assert eng.inputs[0][0].shape[0] == N and drv._gp.X_train_.shape[0] == N       # no lie left in the slot or the estimator
    # ... and the next fit of the real data + one more row extends THIS fit, not one with lies in it
    drv._space.register(Xq[0], 0.3)
    eng.calls.clear()
    drv.suggest_first()
    assert eng.inputs[0][0].shape[0] == N + 1
    assert np.array_equal(eng.inputs[0][0][:N], X)


def test_bookkeeping_advances_once_per_pick():
    q = 4
    drv, eng, X, y = _driver(_policy("ucb", exploration_decay=0.9, exploration_decay_delay=2))
    fn = drv._acquisition_function
    picks = suggest_batch(drv, q)
    assert fn.i == q
    # what q suggest() calls do to kappa: decay at the end of call p once delay <= i
    kappa, used = 2.0, []
    for p in range(1, q + 1):
        used.append(kappa)
        if 2 <= p:
            kappa *= 0.9
    assert fn.kappa == pytest.approx(kappa, rel=0, abs=0)
    kind, ls, noise = _theta(drv._gp)
    want, gaps = B.batch_truth(kind, ls, noise, X, y, eng.Xc, O.UCB, used, "max", q)
    assert gaps.min() >= B.GAP_FLOOR
    assert np.array_equal(B.rows_to_indices(picks, eng.Xc), want)      # pick p used the kappa call p would have used


def test_improvement_policies_take_the_lie_into_y_max():
    drv, eng, X, y = _driver(_policy("ei"))
    suggest_batch(drv, 3, strategy=float(y.max() + 1.0))
    acq_calls = [c for c in eng.calls if c[0] == "acq_argbest"]
    assert len(acq_calls) == 3
    assert drv._acquisition_function.y_max == y.max() + 1.0


def test_engine_calls_of_a_batch():
    q = 5
    drv, eng, _, _ = _driver(_policy("poi"))
    suggest_batch(drv, q)
    names = [c[0] for c in eng.calls]
    assert names.count("posterior") == 1 and names.count("posterior_refresh") == q - 1
    assert names.count("generate_candidates_like") == 1 and names.count("set_candidates") == 0
    assert names.count("fit_append") == q - 1 and names.count("acq_argbest") == q
    assert names.count("fit") == 2 and names[-1] == "fit"            # the theta fit, and the slot put back at the end
    assert "polish_seeds" not in names and "predict_grad" not in names   # no local-search stage
    first_refresh = names.index("posterior_refresh")
    assert names.index("posterior") < first_refresh and names[first_refresh - 1] == "fit_append"


def test_refusals():
    drv, eng, X, y = _driver(_policy("ucb"))
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            suggest_batch(drv, bad)
    with pytest.raises(ValueError, match="strategy"):
        suggest_batch(drv, 2, strategy="median")
    group = B.check_shared_refusals(lambda d: suggest_batch(d, 2), lambda **kw: _driver(_policy("ei"), **kw), "suggest_batch")
    with pytest.raises(NotImplementedError, match="device group"):
        type(group).posterior_refresh(group)
    # another policy
    drv, eng, X, y = _driver(A.GPHedge([_policy("ucb"), _policy("ei")]))
    with pytest.raises(NotImplementedError, match="GPHedge"):
        suggest_batch(drv, 2)

    class Mine(A.UpperConfidenceBound):
        pass

    drv, eng, X, y = _driver(Mine())
    with pytest.raises(NotImplementedError, match="Mine"):
        suggest_batch(drv, 2)


@pytest.mark.skipif(not have_reference(), reason="bayes_opt (the reference) is not importable here")
def test_an_accelerated_bayes_opt_optimizer():
    import_reference()
    from bayes_opt import BayesianOptimization

    from bayesianoptimization_amd import accelerate

    def f(x, y):
        return -(x ** 2) - (y - 1) ** 2 + 1

    pair = []
    for _ in range(2):
        opt = BayesianOptimization(f=f, pbounds={"x": (2, 4), "y": (-3, 3)}, random_state=5, verbose=0)
        eng = RefreshFakeEngine()
        accelerate(opt, engine=eng, lml_on_device=False, n_random=3000)
        opt.maximize(init_points=4, n_iter=2)
        pair.append((opt, eng))
    (a, ea), (b, _) = pair
    picks = suggest_batch(a, 3)
    x_twin = b._acquisition_function.suggest(gp=b._gp, target_space=b._space, n_smart=0, fit_gp=True, random_state=b._random_state)
    assert sorted(picks[0]) == ["x", "y"] and np.array_equal(np.array([picks[0]["x"], picks[0]["y"]]), x_twin)
    assert len({tuple(p.values()) for p in picks}) == 3
    nxt_a, nxt_b = a.suggest(), b.suggest()            # nothing of the batch but the advanced policy: same draw, same fit
    assert a._gp.X_train_.shape[0] == b._gp.X_train_.shape[0] == 6
    # an int parameter: refused
    opt = BayesianOptimization(f=None, pbounds={"x": (2, 4), "k": (0, 5, int)}, random_state=5, verbose=0)
    accelerate(opt, engine=RefreshFakeEngine(), lml_on_device=False)
    opt.register(params={"x": 3.0, "k": 2}, target=1.0)
    with pytest.raises(NotImplementedError, match="transform"):
        suggest_batch(opt, 2)
