"""gpbo_posterior_refresh against the full gpbo_posterior, and a q = 8 suggest_batch against 8 fixed-theta suggest steps, at the C2
(N = 512, d = 8, M = 65 536) and C3 (N = 4096, d = 16, M = 2^20) shapes of BASELINE.json.

    python scripts/batch_refresh_bench.py [--shapes C2,C3] [--warmup 3] [--runs 10] [--out FILE.json]

Protocol: random data (workloads.make_observations, candidates from the device generator), `warmup` untimed
rounds, then the median of `runs` timed ones with min / max beside it; every timing is a host clock around work that ends in a
stream synchronise; everything in ONE process on ONE device, the two sides of each ratio in alternation inside one loop.
Per round of the first loop: fit (N - 1 rows) -> fit_append of row N [timed] -> posterior_refresh [timed; route 1 asserted] -> full
posterior of the same N-row slot [timed].  Second loop: one `suggest(n_smart=0)` at fixed theta [timed: the fixed-theta step] and
one `suggest_batch(q = 8)` [timed] on the same optimizer stand-in over N - 8 real rows, so that the batch ends at N rows.  (Both N are
multiples of 64: an append that crosses the slot's 64-row padding rebuilds the factorisation and its refresh is the full pass — a
batch that starts right at a boundary pays one more full pass than the q - 1 refreshes measured here.)  Prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bayesianoptimization_amd import fused_acquisition as A  # noqa: E402
from bayesianoptimization_amd import suggest_batch  # noqa: E402
from bayesianoptimization_amd import workloads as W  # noqa: E402
from bayesianoptimization_amd.engine import GpEngine  # noqa: E402
from bayesianoptimization_amd.float_space import FloatSpace  # noqa: E402
from bayesianoptimization_amd.gpr import HipGPR  # noqa: E402

Q = 8


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


class Optimizer:
    """what suggest_batch reads of an accelerate()d BayesianOptimization, at FIXED theta (optimizer=None)"""

    def __init__(self, eng, w, X, y):
        from sklearn.gaussian_process.kernels import Matern

        self._random_state = np.random.RandomState(7)
        self._space = FloatSpace(w.pbounds())
        self._space.register_bulk(X, y)
        self._gp = HipGPR(kernel=Matern(nu=2.5, length_scale=w.length_scale), alpha=w.noise, normalize_y=True, optimizer=None,
                          random_state=self._random_state, engine=eng)
        self._acquisition_function = A.UpperConfidenceBound(kappa=2.576)
        self._acquisition_function.default_n_random = w.M

    def step(self):
        return self._acquisition_function.suggest(gp=self._gp, target_space=self._space, n_smart=0, fit_gp=True,
                                                  random_state=self._random_state)


def measure(eng, w, warmup, runs):
    X, y, _ = W.make_observations(w)
    yn, ym, ys = W.normalize_targets(y[:-1])
    yn1, ym1, ys1 = W.normalize_targets(y)
    b = w.bounds_array()
    eng.generate_candidates(w.M, b[:, 0], b[:, 1], 20240601)
    t = {"full_posterior_ms": [], "fit_append_ms": [], "posterior_refresh_ms": []}

    def timed(key, fn, keep):
        t0 = time.perf_counter()
        out = fn()
        eng.synchronize()
        if keep:
            t[key].append((time.perf_counter() - t0) * 1e3)
        return out

    for r in range(warmup + runs):
        keep = r >= warmup
        eng.fit(X[:-1], yn, w.kernel, w.length_scale, w.noise)
        eng.posterior(0, ym, ys, fetch=False)
        eng.synchronize()
        timed("fit_append_ms", lambda: eng.fit_append(X[-1:], yn1), keep)
        route = timed("posterior_refresh_ms", lambda: eng.posterior_refresh(0, ym1, ys1, fetch=False, return_route=True), keep)[2]
        if route != 1:
            raise RuntimeError("posterior_refresh did not take the incremental route")
        timed("full_posterior_ms", lambda: eng.posterior(0, ym1, ys1, fetch=False), keep)
    opt = Optimizer(eng, w, X[:-Q], y[:-Q])
    step_ms, batch_ms = [], []
    for r in range(warmup + runs):
        t0 = time.perf_counter()
        opt.step()
        eng.synchronize()
        t1 = time.perf_counter()
        picks = suggest_batch(opt, Q)
        eng.synchronize()
        t2 = time.perf_counter()
        if len(picks) != Q:
            raise RuntimeError("suggest_batch returned the wrong number of picks")
        if r >= warmup:
            step_ms.append((t1 - t0) * 1e3)
            batch_ms.append((t2 - t1) * 1e3)
    out = {k: stats(v) for k, v in t.items()}
    out["refresh_over_full"] = out["posterior_refresh_ms"]["median"] / out["full_posterior_ms"]["median"]
    out["fixed_theta_step_ms"] = stats(step_ms)
    out[f"suggest_batch_q{Q}_ms"] = stats(batch_ms)
    out[f"{Q}_steps_over_batch"] = Q * out["fixed_theta_step_ms"]["median"] / out[f"suggest_batch_q{Q}_ms"]["median"]
    out["shape"] = {"N": w.N, "batch_real_rows": w.N - Q, "d": w.d, "M": w.M, "kernel": W.KERNEL_NAMES[w.kernel], "length_scale": w.length_scale}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C2,C3")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs, "q": Q, "clock": "host perf_counter around call + stream synchronise"}}
    with GpEngine(0) as eng:
        out["device"] = eng.device_info().get("name")
        for name in args.shapes.split(","):
            out[name] = measure(eng, W.ALL[name], args.warmup, args.runs)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
