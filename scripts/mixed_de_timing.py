"""The mixed-space differential evolution: the device walk (gpbo_evolve_mixed, csrc/evolve.hip) against SciPy's solver over the
host objective (one device round trip per trial), on libgpbo_dbg.so.

    python scripts/mixed_de_timing.py      # writes profiles/mixed_de_timing.json

* per evaluation: microseconds of the device objective inside one launch (gpbo_debug_evolve_eval over 512 points, less a one-point
  call) and of the host objective the reference-shaped path calls (_get_acq over _posterior_trusted, one point), at N in
  {16, 64, 128, 256, 512} and D in {5, 16};
* per suggest(): wall milliseconds with device_evolve False (SciPy) and True (the device walk) on three mixed spaces, the median of
  5 after one warm-up, with the walk's nit / nfev and whether the two suggestions and RandomStates agree.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sklearn.gaussian_process.kernels import Matern  # noqa: E402

from bayesianoptimization_amd import fused_acquisition as A  # noqa: E402
from bayesianoptimization_amd.engine import GpEngine  # noqa: E402
from bayesianoptimization_amd.float_space import MixedSpace  # noqa: E402
from bayesianoptimization_amd.gpr import HipGPR  # noqa: E402

SPACES = {
    5: {"f0": (0.0, 2.0), "f1": (-1.0, 1.0), "f2": (3.0, 4.0), "i0": (-3, 7, int), "i1": (0, 4, int)},
    16: {**{f"f{j}": (0.0, 1.0 + j) for j in range(12)}, "i0": (-3, 7, int), "c": ("x", "y", "z")},
}
SUGGEST_SPACES = {
    "float_int_cat5": {"a": (0.0, 2.0), "n": (-3, 7, int), "c": ("x", "y", "z")},
    "mixed8": {"a": (0.0, 2.0), "n": (-3, 7, int), "b": (1.0, 4.0), "c": ("x", "y", "z"), "e": (5.0, 6.0), "k": (0, 1, int)},
    "wide16": SPACES[16],
}


def _model(eng, pb, N, seed):
    sp = MixedSpace(pb)
    X = sp.random_sample(N, np.random.RandomState(seed))
    y = np.sin(X.sum(axis=1)) + 0.1 * X[:, 0]
    sp.register_bulk(X, y)
    gp = HipGPR(kernel=Matern(nu=2.5, length_scale=1.3), alpha=1e-6, normalize_y=True, optimizer=None, engine=eng,
                transform=sp.kernel_transform)
    return sp, gp


def per_eval(eng):
    rows = []
    for D, pb in SPACES.items():
        for N in (16, 64, 128, 256, 512):
            sp, gp = _model(eng, pb, N, N)
            gp.fit(sp.params, sp.target)
            groups = A._mixed_space_groups([gp], sp, np.random.RandomState(0))
            fn = A.UpperConfidenceBound(kappa=2.576)
            args = (fn._acq_kind, fn._acq_param(), 0.0, float(gp._y_train_mean), float(gp._y_train_std), groups)
            pts = sp.random_sample(512, np.random.RandomState(1))
            t_one, t_all = [], []
            for _ in range(5):
                t0 = time.perf_counter()
                eng.debug_evolve_eval(*args, pts[:1])
                t_one.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                eng.debug_evolve_eval(*args, pts)
                t_all.append(time.perf_counter() - t0)
            dev_us = (min(t_all) - min(t_one)) / 511 * 1e6
            obj = fn._get_acq(gp)
            obj(pts[0])
            t0 = time.perf_counter()
            for p in pts[:200]:
                obj(p)
            host_us = (time.perf_counter() - t0) / 200 * 1e6
            rows.append({"N": N, "D": sp.dim, "device_us_per_eval": round(dev_us, 2), "host_objective_us_per_call": round(host_us, 2)})
            print(rows[-1], file=sys.stderr)
    return rows


def per_suggest(eng):
    rows = []
    for name, pb in SUGGEST_SPACES.items():
        for N in (30, 200):
            res = {}
            for device in (False, True):
                sp, gp = _model(eng, pb, N, 3)
                fn = A.UpperConfidenceBound(kappa=2.576)
                fn.device_evolve = device
                walk = []
                orig = eng.evolve_mixed
                eng.evolve_mixed = lambda *a, _o=orig, **k: (lambda r: (walk.append(r[2:4]), r)[1])(_o(*a, **k))
                ts, xs = [], []
                try:
                    for rep in range(6):
                        rs = np.random.RandomState(50 + rep)
                        t0 = time.perf_counter()
                        xs.append(fn.suggest(gp, sp, n_random=10_000, n_smart=10, random_state=rs))
                        ts.append(time.perf_counter() - t0)
                        xs.append(rs.get_state(legacy=True)[2])
                finally:
                    del eng.evolve_mixed
                res[device] = (float(np.median(ts[1:])) * 1e3, xs, walk)
            nit_nfev = res[True][2][-1] if res[True][2] else None
            same = all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(res[False][1], res[True][1]))
            rows.append({"space": name, "D": MixedSpace(pb).dim, "N": N, "host_de_ms": round(res[False][0], 3),
                         "device_de_ms": round(res[True][0], 3), "nit": None if nit_nfev is None else int(nit_nfev[0]),
                         "nfev": None if nit_nfev is None else int(nit_nfev[1]), "same_suggestions_and_rng": bool(same)})
            print(rows[-1], file=sys.stderr)
    return rows


def main():
    with GpEngine(0, debug=True) as eng:
        eng.set_timing(False)
        out = {"per_evaluation": per_eval(eng), "per_suggest": per_suggest(eng)}
    path = os.path.join(ROOT, "profiles", "mixed_de_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
