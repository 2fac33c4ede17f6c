"""CPU: the frame suggest_batch / suggest_thompson / suggest_mes share (bayesianoptimization_amd/_suggest.py), held to what the commit
BEFORE the frame existed did — tests/suggest_frame_parent.json, recorded from that commit by this module itself:

    python tests/test_suggest_frame_host.py --record PATH        (in a checkout of the parent, this file copied into its tests/)

  * refusals: every driver state x every argument set of each function — which exception wins and what it says, or that there is
    none, and the engine's call log afterwards;
  * replay: the calls of the three functions over the engine doubles — the engine call log, the returned parameters bit for bit, the
    info dict, the RandomState left behind, the policy's bookkeeping.
The recorder uses the public functions and the test doubles only, so that it runs on the parent's tree unchanged; that is also why
it brings its own data.  The third part is a truth test, not a recording: the three functions on a scaled model
(ConstantKernel * k + WhiteKernel), the noise of whose draws, floor and appends is alpha + white."""
import hashlib
import itertools
import json
import os
import sys
import warnings

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pytest

import batch_truth as B
import matern_family_truth as F
import paths_ascent_truth as PA
import paths_truth as P
import scaled_kernel_truth as SK
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import suggest_batch, suggest_mes, suggest_thompson
from bayesianoptimization_amd.engine import GroupEngine
from bayesianoptimization_amd.thompson import spectral_draw
from helpers import FakeEngine
from test_log_ei_host import LogEiFakeEngine
from test_mes_host import MesFakeEngine
from test_suggest_batch_host import RefreshFakeEngine

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "suggest_frame_parent.json")
D, N, M, FEATURES = 3, 30, 1500, 32
BOUNDS = np.array([[0.0, 1.0], [-1.0, 2.0], [0.5, 1.5]])
FUNCTIONS = {"thompson": suggest_thompson, "mes": suggest_mes, "batch": suggest_batch}


def data():
    X, y = F.data(N, D, seed=0)
    return BOUNDS[:, 0] + X * (BOUNDS[:, 1] - BOUNDS[:, 0]), y


class Mine(A.UpperConfidenceBound):
    pass


POLICIES = {"ucb": lambda: A.UpperConfidenceBound(kappa=2.0, exploration_decay=0.9, exploration_decay_delay=0),
            "ei": lambda: A.ExpectedImprovement(xi=0.01), "poi": lambda: A.ProbabilityOfImprovement(xi=0.5),
            "log_ei": lambda: A.LogExpectedImprovement(xi=0.01),
            "hedge": lambda: A.GPHedge([A.UpperConfidenceBound(kappa=2.0), A.ExpectedImprovement(xi=0.01)]), "mine": Mine}


def driver(engine, policy="ucb", seed=3, **kw):
    X, y = data()
    kw.setdefault("lml_on_device", False)
    return B.Driver(engine, X, y, BOUNDS, POLICIES[policy](), seed=seed, n_random=M, **kw)


# ---- digests ---------------------------------------------------------------------------------------------------------------------
def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode() + a.tobytes())
    return h.hexdigest()[:24]


def plain(v):
    """`v` as JSON gives it back"""
    return json.loads(json.dumps(v))


def rows(picks):
    picks = picks if isinstance(picks, list) else [picks]
    return [list(p) for p in picks], np.array([list(p.values()) for p in picks], dtype=np.float64)


def state_of(drv):
    name, key, pos, has_gauss, cached = drv._random_state.get_state()
    fn = drv._acquisition_function
    param = getattr(fn, "kappa", getattr(fn, "xi", None))
    y_max = getattr(fn, "y_max", None)
    return {"random_state": [name, sha(key), int(pos), int(has_gauss), float(cached).hex()],
            "policy": [int(fn.i), None if param is None else float(param).hex(), None if y_max is None else float(y_max).hex()]}


# ---- part 1: the refusal table -----------------------------------------------------------------------------------------------------
class NoSample(F.FamilyFakeEngine):
    mes_argbest = MesFakeEngine.mes_argbest


class NoAscent(P.PathsFakeEngine):
    mes_argbest = MesFakeEngine.mes_argbest


#: function -> (the double it runs on, {a call it needs: a double without it})
ENGINES = {"thompson": (PA.AscentFakeEngine, {"sample_paths": F.FamilyFakeEngine, "ascend_paths": P.PathsFakeEngine}),
           "mes": (MesFakeEngine, {"sample_paths": NoSample, "mes_argbest": PA.AscentFakeEngine, "ascend_paths": NoAscent}),
           "batch": (RefreshFakeEngine, {"posterior_refresh": FakeEngine})}
STATES = ("fine", "gp_object", "slot_1", "empty", "constraint", "transform", "group", "host_kernel")

#: the argument sets: fine first, then each invalid value the functions' own tests use ("policy": the driver's, not the call's)
_SMALL = {"n_random": M, "n_features": 16}
_REFINE = [{"refine": v} for v in (-1, 9, 1.5, True)]
ARGS = {
    "thompson": [{"q": 2, **_SMALL}, {"q": 2, "refine": 2, **_SMALL}] + [{"q": v} for v in (0, -1, 1.5, True)]
    + [{"q": 2, **kw} for kw in [{"n_features": 0}, {"n_features": 4097}, {"n_random": 0}] + _REFINE],
    "mes": [{"n_samples": 2, "refine": 0, **_SMALL}, {"n_samples": 2, "refine": 1, **_SMALL}]
    + [{"n_samples": v} for v in (0, -1, 65, 1.5, True, None)]
    + [{"n_samples": 2, **kw} for kw in [{"n_features": 0}, {"n_features": 4097}, {"n_random": 0}, {"floor_sigmas": -0.5},
                                         {"floor_sigmas": float("nan")}, {"floor_sigmas": float("inf")}] + _REFINE],
    "batch": [{"q": 2}] + [{"q": v} for v in (0, -1, 1.5, True)]
    + [{"q": 2, "strategy": "median"}, {"q": 2, "policy": "hedge"}, {"q": 2, "policy": "mine"},
       {"q": 2, "policy": "hedge", "strategy": "median"}, {"q": True, "policy": "mine"}],
}


def broken_driver(name, state, policy):
    """(driver, the engine whose call log counts) in one of STATES or "lacks:<call>" """
    from sklearn.gaussian_process.kernels import RationalQuadratic

    from bayesianoptimization_amd.constraint_model import HipConstraintModel
    from bayesianoptimization_amd.float_space import FloatSpace, MixedSpace

    cls, lacking = ENGINES[name]
    eng = lacking[state[6:]]() if state.startswith("lacks:") else cls()
    drv = driver(eng, policy, **({"kernel": RationalQuadratic()} if state == "host_kernel" else {}))
    empty = {f"x{j}": tuple(b) for j, b in enumerate(BOUNDS)}
    if state == "gp_object":
        drv._gp = object()
    elif state == "slot_1":
        drv._gp.slot = 1
    elif state == "empty":
        drv._space = FloatSpace(empty)
    elif state == "constraint":
        X, y = data()
        cm = HipConstraintModel(None, np.array([-np.inf]), np.array([0.5]), engine=eng, random_state=np.random.RandomState(3))
        drv._space = FloatSpace(empty, constraint=cm)
        drv._space.register_bulk(X, y, np.cos(X.sum(1)))
    elif state == "transform":
        drv._gp.transform = MixedSpace({"x0": (0.0, 1.0), "x1": (-1, 2, int), "x2": (0.5, 1.5)}).kernel_transform
    elif state == "group":
        drv._gp.engine = object.__new__(GroupEngine)          # (no devices opened: the type is what is refused)
        drv._gp.engine.__dict__.update(_g=None, _h=None)
    return drv, eng


def refusal_cases():
    for name in FUNCTIONS:
        states = STATES + tuple(f"lacks:{c}" for c in ENGINES[name][1])
        for state, args in itertools.product(states, ARGS[name]):
            yield f"{name} | {state} | {args!r}", name, state, args


def run_refusal(name, state, args):
    args = dict(args)
    drv, eng = broken_driver(name, state, args.pop("policy", "ucb"))
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            FUNCTIONS[name](drv, **args)
        outcome = ["", "no exception"]
    except Exception as e:  # noqa: BLE001
        outcome = [type(e).__name__, str(e)]
    return plain({"outcome": outcome, "calls": eng.calls})


# ---- part 2: the replay ------------------------------------------------------------------------------------------------------------
def replay_cases():
    """(id, function, engine double, policy, arguments); a real engine runs the same list (the doubles' names are then unused)"""
    for q, refine in itertools.product((1, 16, 17), (0, 2)):
        yield (f"thompson q={q} refine={refine}", "thompson", PA.AscentFakeEngine if refine else P.PathsFakeEngine, "ucb",
               {"q": q, "n_random": M, "n_features": FEATURES, "refine": refine})
    for n, refine in itertools.product((1, 3, 17), (0, 1)):
        yield (f"mes n_samples={n} refine={refine}", "mes", MesFakeEngine, "ucb",
               {"n_samples": n, "n_random": M, "n_features": FEATURES, "refine": refine, "return_info": True})
    for q, policy, strategy in itertools.product((1, 3), ("ucb", "ei", "poi", "log_ei"), ("max", "min", 0.25)):
        yield (f"batch q={q} {policy} {strategy}", "batch", LogEiFakeEngine if policy == "log_ei" else RefreshFakeEngine, policy,
               {"q": q, "strategy": strategy})


def run_replay(name, drv, args):
    """The call's results as arrays: what a run on a real engine compares too"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = FUNCTIONS[name](drv, **args)
    info = {}
    if name == "mes":
        out, info = out
    keys, values = rows(out)
    return {"keys": keys, "values": values, "info": info, **state_of(drv)}


def digest_replay(res, calls):
    info = {k: (sha(v) if isinstance(v, np.ndarray) else float(v).hex() if isinstance(v, float) else v) for k, v in res["info"].items()}
    return plain({"calls": calls, "keys": res["keys"], "values": sha(res["values"]), "info": info,
                  "random_state": res["random_state"], "policy": res["policy"]})


def record_all():
    out = {"refusals": {}, "replay": {}}
    for cid, name, state, args in refusal_cases():
        out["refusals"][cid] = run_refusal(name, state, args)
    for cid, name, cls, policy, args in replay_cases():
        eng = cls()
        out["replay"][cid] = digest_replay(run_replay(name, driver(eng, policy), args), eng.calls)
    return out


@pytest.fixture(scope="module")
def parent():
    with open(RECORD) as f:
        return json.load(f)


def test_the_record_names_its_commit_and_covers_every_case(parent):
    assert len(parent["header"]["parent"]) == 40 and "--record" in parent["header"]["command"]
    assert sorted(parent["refusals"]) == sorted(c[0] for c in refusal_cases())
    assert sorted(parent["replay"]) == sorted(c[0] for c in replay_cases())
    # the table is about refusals: most cases raise, the fine ones do not, and all three exception families are there
    kinds = {v["outcome"][0] for v in parent["refusals"].values()}
    assert {"", "ValueError", "NotImplementedError", "TargetSpaceEmptyError", "ConstraintNotSupportedError"} <= kinds


@pytest.mark.parametrize("name", list(FUNCTIONS))
def test_refusals_are_the_parents(parent, name):
    """Which exception wins, its text, and the engine's call log — a case that does not raise stays one that does not."""
    wrong = []
    for cid, fname, state, args in refusal_cases():
        if fname == name:
            got = run_refusal(fname, state, args)
            if got != parent["refusals"][cid]:
                wrong.append((cid, got, parent["refusals"][cid]))
    assert not wrong, f"{len(wrong)} cases differ from the parent; the first: {wrong[0]}"


@pytest.mark.parametrize("case", list(replay_cases()), ids=lambda c: c[0])
def test_replay_is_the_parents(parent, case):
    cid, name, cls, policy, args = case
    eng = cls()
    got = digest_replay(run_replay(name, driver(eng, policy), args), eng.calls)
    assert got == parent["replay"][cid]


# ---- part 3: a scaled model --------------------------------------------------------------------------------------------------------
class ScaledRecordingEngine(SK.ScaledFakeEngine):
    """scaled_kernel_truth.ScaledFakeEngine (TEST DOUBLE ONLY) + stubs of the four calls the suggest functions make beyond a policy's
    suggest: they record what they were handed and answer with fixed values (every draw's maximum far below the data)."""
    LOW = -1e9

    def __init__(self):
        super().__init__()
        self.eps, self.y_star = [], None

    def sample_paths(self, omega, phase, weights, eps, slot=0, y_mean=0.0, y_std=1.0, index_offset=0, return_values=False):
        self.calls.append(("sample_paths", slot, np.shape(weights)[0]))
        self.eps.append(np.array(eps))
        S = np.shape(weights)[0]
        return np.arange(S, dtype=np.int64), np.full(S, self.LOW), None

    def ascend_paths(self, omega, phase, weights, eps, box_lo, box_hi, n_starts=4, **kw):
        self.calls.append(("ascend_paths", kw.get("slot", 0), np.shape(weights)[0]))
        self.eps.append(np.array(eps))
        S, d = np.shape(weights)[0], len(box_lo)
        x = np.broadcast_to(np.asarray(box_lo, dtype=np.float64), (S, n_starts, d)).copy()
        return {"x": x, "f": np.full((S, n_starts), self.LOW), "winner": np.zeros(S, dtype=np.int64), "x_best": x[:, 0],
                "best_val": np.full(S, self.LOW)}

    def mes_argbest(self, y_star, k_seeds=0, index_offset=0, return_values=False):
        self.calls.append(("mes_argbest", len(y_star), k_seeds))
        self.y_star = np.array(y_star)
        return 0, -1.0, np.empty(0, dtype=np.int64), np.empty(0), None

    def posterior_refresh(self, slot=0, y_mean=0.0, y_std=1.0, fetch=True, return_route=False):
        self.calls.append(("posterior_refresh", slot))
        return self.posterior(slot, y_mean, y_std, fetch)


def scaled_driver(policy="ucb"):
    from sklearn.gaussian_process.kernels import ConstantKernel, Matern, WhiteKernel

    eng = ScaledRecordingEngine()
    return driver(eng, policy, kernel=ConstantKernel(2.0) * Matern(nu=2.5) + WhiteKernel(1e-2), scaled_kernels=True), eng


def twin_draws(n_draws):
    """The documented draws, replayed by hand on a twin: (the twin's gp, per group the unit normal draws behind eps)"""
    twin, teng = scaled_driver()
    gp, rng = twin._gp, twin._random_state
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp.fit(twin._space.params, twin._space.target)
    teng.generate_candidates_like(M, BOUNDS[:, 0], BOUNDS[:, 1], rng)
    z = []
    for first in range(0, n_draws, 16):
        S = min(16, n_draws - first)
        spectral_draw(gp._kind, FEATURES, D, rng)
        rng.standard_normal((S, FEATURES))
        z.append(rng.standard_normal((S, N)))
    return twin, gp, z


@pytest.mark.parametrize("name,refine", [("thompson", 0), ("thompson", 2), ("mes", 0), ("mes", 1)])
def test_a_scaled_models_noise_is_alpha_plus_white(name, refine):
    n_draws = 17
    drv, eng = scaled_driver()
    args = {"n_random": M, "n_features": FEATURES, "refine": refine}
    if name == "mes":
        _params, info = suggest_mes(drv, n_draws, floor_sigmas=3.0, return_info=True, **args)
    else:
        assert len(suggest_thompson(drv, n_draws, **args)) == n_draws
    twin, gp, z = twin_draws(n_draws)
    assert not drv._gp._host_mode and drv._gp._scale is not None and drv._gp._scale == gp._scale
    alpha, (amplitude, white) = float(gp.alpha), gp._scale
    assert white > 0.0 and amplitude != 1.0
    assert [c[2] for c in eng.calls if c[0] == ("ascend_paths" if refine else "sample_paths")] == [16, 1] and len(eng.eps) == 2
    for got, unit in zip(eng.eps, z):
        assert np.array_equal(got, unit * np.sqrt(alpha + white))
        assert not np.array_equal(got, unit * np.sqrt(alpha))
    assert state_of(drv)["random_state"] == state_of(twin)["random_state"]
    if name == "mes":
        # every stub draw ends far below the data: y* is the floor, 3 noise standard deviations above the best observation
        floor = float(np.max(drv._space.target)) + 3.0 * np.sqrt(alpha + white) * float(gp._y_train_std)
        assert np.array_equal(info["y_star"], np.full(n_draws, floor)) and np.array_equal(eng.y_star, info["y_star"])
        assert floor != float(np.max(drv._space.target)) + 3.0 * np.sqrt(alpha) * float(gp._y_train_std)


@pytest.mark.parametrize("policy", ["ucb", "ei"])
def test_a_scaled_models_appends_carry_amplitude_and_white(policy):
    q = 4
    drv, eng = scaled_driver(policy)
    picks = suggest_batch(drv, q)
    assert len(picks) == q and not drv._gp._host_mode
    amplitude, white = drv._gp._scale
    appends = [c for c in eng.scaled_calls if c[0] == "fit_append"]
    assert [c[0] for c in eng.calls].count("fit_append") == q - 1 == len(appends)
    assert all(c[1:] == (float(amplitude), float(white)) for c in appends) and white > 0.0 and amplitude != 1.0
    assert [c[0] for c in eng.calls].count("posterior_refresh") == q - 1


if __name__ == "__main__":
    import subprocess

    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_suggest_frame_host.py --record PATH")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=root, capture_output=True, text=True, check=True).stdout.strip()
    table = {"header": {"parent": head, "command": "python tests/test_suggest_frame_host.py --record PATH",
                        "what": "recorded in a checkout of `parent` with this module copied into its tests/"}, **record_all()}
    with open(sys.argv[2], "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(table['refusals'])} refusal cases and {len(table['replay'])} replay cases of {head} -> {sys.argv[2]}")
