"""gpbo_sample_paths — 16 posterior function draws over the resident candidates and their maximisers — next to the full
gpbo_posterior and a one-row gpbo_posterior_refresh, at the C2 (N = 512, d = 8, M = 65 536) and C3 (N = 4096, d = 16, M = 2^20)
shapes of BASELINE.json.

    python scripts/sample_paths_bench.py [--shapes C2,C3] [--features 1024] [--warmup 3] [--runs 10] [--out FILE.json]

Protocol: random data (workloads.make_observations, candidates from the device generator), `warmup` untimed rounds,
then the median of `runs` timed ones with min / max beside it; every timing is a host clock around a call that ends in a stream
synchronise (the uploads of the call's draws and the fetch of its 16 picks are inside: it is what a caller waits for); everything in
ONE process on ONE device, all timed calls in alternation inside one loop.  Per round: fit (N - 1 rows) -> full posterior -> fit_append
of row N -> posterior_refresh [timed; route 1 asserted] -> full posterior of the N-row slot [timed] -> sample_paths, 16 paths, F
features [timed] -> the same with ONE feature [timed: the training-point phase, the path weights, the 16 selections and the call's
fixed costs; the difference to the line before is the feature phase] -> one path, F features [timed].  Prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bayesianoptimization_amd import workloads as W  # noqa: E402
from bayesianoptimization_amd.engine import GpEngine  # noqa: E402
from bayesianoptimization_amd.thompson import spectral_draw  # noqa: E402

S = 16


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def measure(eng, w, features, warmup, runs):
    X, y, _ = W.make_observations(w)
    yn, ym, ys = W.normalize_targets(y[:-1])
    yn1, ym1, ys1 = W.normalize_targets(y)
    b = w.bounds_array()
    eng.generate_candidates(w.M, b[:, 0], b[:, 1], 20240601)
    rs = np.random.RandomState(11)
    omega, phase = spectral_draw(w.kernel, features, w.d, rs)
    weights = rs.standard_normal((S, features))
    eps = rs.standard_normal((S, w.N)) * np.sqrt(w.noise)
    keys = ("posterior_refresh_ms", "full_posterior_ms", "sample_paths_16_ms", "sample_paths_16_one_feature_ms", "sample_paths_1_ms")
    t = {k: [] for k in keys}

    def timed(key, fn, keep):
        t0 = time.perf_counter()
        out = fn()
        eng.synchronize()
        if keep:
            t[key].append((time.perf_counter() - t0) * 1e3)
        return out

    picks = None
    for r in range(warmup + runs):
        keep = r >= warmup
        eng.fit(X[:-1], yn, w.kernel, w.length_scale, w.noise)
        eng.posterior(0, ym, ys, fetch=False)
        eng.fit_append(X[-1:], yn1)
        eng.synchronize()
        route = timed("posterior_refresh_ms", lambda: eng.posterior_refresh(0, ym1, ys1, fetch=False, return_route=True), keep)[2]
        if route != 1:
            raise RuntimeError("posterior_refresh did not take the incremental route")
        timed("full_posterior_ms", lambda: eng.posterior(0, ym1, ys1, fetch=False), keep)
        best = timed("sample_paths_16_ms", lambda: eng.sample_paths(omega, phase, weights, eps, y_mean=ym1, y_std=ys1), keep)[0]
        timed("sample_paths_16_one_feature_ms",
              lambda: eng.sample_paths(omega[:1], phase[:1], weights[:, :1], eps, y_mean=ym1, y_std=ys1), keep)
        timed("sample_paths_1_ms", lambda: eng.sample_paths(omega, phase, weights[:1], eps[:1], y_mean=ym1, y_std=ys1), keep)
        if picks is not None and not np.array_equal(picks, best):
            raise RuntimeError("sample_paths is not repeatable")
        picks = best
    out = {k: stats(v) for k, v in t.items()}
    full = out["sample_paths_16_ms"]["median"]
    out["feature_phase_ms"] = full - out["sample_paths_16_one_feature_ms"]["median"]
    out["paths_over_full_posterior"] = full / out["full_posterior_ms"]["median"]
    out["paths_over_refresh"] = full / out["posterior_refresh_ms"]["median"]
    out["distinct_picks_of_16"] = int(np.unique(picks).shape[0])
    out["shape"] = {"N": w.N, "d": w.d, "M": w.M, "F": features, "paths": S, "kernel": W.KERNEL_NAMES[w.kernel],
                    "length_scale": w.length_scale}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C2,C3")
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs, "paths": S, "features": args.features,
                        "clock": "host perf_counter around call + stream synchronise"}}
    with GpEngine(0) as eng:
        out["device"] = eng.device_info().get("name")
        for name in args.shapes.split(","):
            out[name] = measure(eng, W.ALL[name], args.features, args.warmup, args.runs)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
