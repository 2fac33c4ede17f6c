"""What the reference's host-side objects return, for the CPU tests that hold this package's stand-ins to them (test
infrastructure; runs where the reference is importable, see oracle/refenv.py).

    python -m oracle.gen_reference_host            -> tests/golden/reference_host.npz

tests/test_host_logic.py and tests/test_mixed_space_host.py compare FloatSpace / MixedSpace / fused_acquisition with the
numbers stored here, so that they run from the repository alone:
  cand_<C>, bounds_<C>         TargetSpace(None, pbounds).random_sample(777, RandomState(7)) and .bounds for C1, C2, C5S
  orch_<kind>_<n_smart>_*      two suggest() calls of bayes_opt's UCB / EI / POI over the P1 history (plain sklearn GP,
                               RandomState(11)): the points, the next uniform() of the stream, .i, get_acquisition_params()
  mixed_*                      TargetSpace over a float / int / categorical space: keys, bounds, masks, samples, the stream
                               position after each, kernel_transform, parameter kinds, and the device column groups
A fixture is data: inputs and expected outputs, no source text.
"""
from __future__ import annotations

import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bayesianoptimization_amd import fused_acquisition as A  # noqa: E402
from bayesianoptimization_amd import workloads as W  # noqa: E402
from oracle.refenv import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reference_host.npz")
CAND_CONFIGS = ("C1", "C2", "C5S")
ORCH_KINDS = ("ucb", "ei", "poi")
ORCH_N_SMART = (0, 3)
MIXED_N = (0, 1, 7, 5000)


def text(obj) -> np.ndarray:
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def untext(a) -> object:
    return json.loads(bytes(np.asarray(a, dtype=np.uint8)).decode())


def _candidates(out):
    from bayes_opt.target_space import TargetSpace

    for name in CAND_CONFIGS:
        w = getattr(W, name)
        ts = TargetSpace(None, w.pbounds())
        out[f"cand_{name}"] = ts.random_sample(777, np.random.RandomState(7))
        out[f"bounds_{name}"] = ts.bounds


def _orchestration(out):
    from bayes_opt import acquisition as RA
    from bayes_opt.target_space import TargetSpace
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import Matern

    w = W.P1
    X, y, _ = W.make_observations(w)
    X, y = X[:40], y[:40]
    for kind in ORCH_KINDS:
        for n_smart in ORCH_N_SMART:
            ts = TargetSpace(None, w.pbounds())
            for i in range(len(y)):
                ts.register(X[i], y[i])
            ref = {"ucb": RA.UpperConfidenceBound(kappa=1.7, exploration_decay=0.9), "ei": RA.ExpectedImprovement(xi=0.02),
                   "poi": RA.ProbabilityOfImprovement(xi=0.02)}[kind]
            rs = np.random.RandomState(11)
            gp = GaussianProcessRegressor(kernel=Matern(nu=2.5, length_scale=0.4), alpha=1e-6, normalize_y=True, optimizer=None)
            xs = [ref.suggest(gp, ts, n_random=500, n_smart=n_smart, random_state=rs) for _ in range(2)]
            key = f"orch_{kind}_{n_smart}"
            out[key + "_x"] = np.array(xs)
            out[key + "_next_uniform"] = np.array([rs.uniform()])
            out[key + "_i"] = np.array([ref.i])
            out[key + "_params"] = text(ref.get_acquisition_params())


def _mixed(out):
    from bayes_opt.target_space import TargetSpace
    from test_mixed_space_host import PB, _engine_over, _Gp, _NumpyLib

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ts = TargetSpace(None, PB)
    out["mixed_keys"] = text(list(ts.keys))
    out["mixed_dim"] = np.array([ts.dim])
    out["mixed_bounds"] = ts.bounds
    for k in ts.keys:
        out[f"mixed_mask_{k}"] = np.asarray(ts.masks[k])
    out["mixed_continuous_dimensions"] = np.asarray(ts.continuous_dimensions)
    out["mixed_param_types"] = text({k: type(ts._params_config[k]).__name__ for k in ts.keys})
    for n in MIXED_N:
        rs = np.random.RandomState(5)
        a = ts.random_sample(n, rs)
        out[f"mixed_sample_{n}"] = a
        out[f"mixed_sample_{n}_next_uniform"] = np.array([rs.uniform()])
        out[f"mixed_transform_{n}"] = ts.kernel_transform(a)
    g = A._mixed_groups_on_device([_Gp(_engine_over(_NumpyLib()), ts.kernel_transform)], ts, np.random.RandomState(0), 10**5)
    assert g is not None, "the reference's TargetSpace no longer qualifies for the device assembly"
    out["mixed_groups"] = text([[gi[0], int(gi[1]), int(gi[2])] for gi in g])
    for j, gi in enumerate(g):
        out[f"mixed_group_{j}_lo"] = np.asarray(gi[3], dtype=np.float64)
        out[f"mixed_group_{j}_hi"] = np.asarray(gi[4], dtype=np.float64)
    rs = np.random.RandomState(9)
    out["mixed_sample_3000_seed9"] = ts.random_sample(3000, rs)
    out["mixed_sample_3000_seed9_next_uniform"] = np.array([rs.uniform()])


def generate(path=OUT):
    import_reference()
    out = {}
    _candidates(out)
    _orchestration(out)
    _mixed(out)
    np.savez_compressed(path, **out)
    return path


if __name__ == "__main__":
    print(generate())
