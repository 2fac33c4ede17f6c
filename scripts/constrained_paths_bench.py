"""gpbo_sample_paths_constrained — 16 draws of the objective and of C constraints over the candidates, the violation folded and
the constrained pick made on the device — next to what a user could do before it and next to its compute floor, at the C3 shape of
BASELINE.json (N = 4096, d = 16, M = 2^20), S = 16, F = 1024, C = 1 and 2.

    python scripts/constrained_paths_bench.py [--constraints 1,2] [--features 1024] [--warmup 3] [--runs 10] [--out FILE.json]

Protocol: random data (workloads.make_observations; constraint j's targets are the objective's rolled by 7 j rows,
candidates from the device generator), every slot fitted at the shape's fixed theta, `warmup` untimed rounds, then the median of
`runs` timed ones with min / max beside it; every timing is a host clock around calls that end in a stream synchronise (uploads and
fetches inside); ONE process, ONE device, the three timed routes in alternation inside one loop.  Per round:
  constrained_ms   one sample_paths_constrained call, nothing fetched but the picks;
  host_rule_ms     1 + C sample_paths calls with the values fetched ((1 + C) x 16 x M doubles through the host) and the rule of
                   include/gpbo.h applied in NumPy: what a user could do before the call existed [the same picks asserted];
  floor_ms         the same 1 + C sample_paths calls without the fetch: the draws' arithmetic and their selections alone.
`over_floor` = constrained / floor, `host_rule_over_constrained` = host_rule / constrained (medians).  ub_j = the median of the
first round's values of constraint j, lb_j = -inf: about half the candidates pass each constraint.  Prints one JSON object.
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


def host_rule(values, lb, ub, y_std):
    """(idx, val, viol, feasible) by the rule of include/gpbo.h from values (1 + C, S, M); no NaN among them"""
    total = None
    for j in range(1, values.shape[0]):
        c = values[j]
        t = np.maximum(np.maximum(lb[j - 1] - c, c - ub[j - 1]), 0.0) / y_std[j]
        total = t if total is None else total + t
    ok = total == 0.0
    any_ok = ok.any(axis=1)
    idx = np.where(any_ok, np.argmax(np.where(ok, values[0], -np.inf), axis=1), np.argmin(total, axis=1))
    rows = np.arange(values.shape[1])
    return idx, values[0][rows, idx], total[rows, idx], any_ok


def measure(eng, w, C, features, warmup, runs):
    X, y, _ = W.make_observations(w)
    b = w.bounds_array()
    lo, hi = np.ascontiguousarray(b[:, 0]), np.ascontiguousarray(b[:, 1])
    eng.generate_candidates(w.M, lo, hi, 20240601)
    rs = np.random.RandomState(11)
    y_mean, y_std, draws = np.empty(1 + C), np.empty(1 + C), []
    for j in range(1 + C):
        yn, y_mean[j], y_std[j] = W.normalize_targets(np.roll(y, 7 * j))
        eng.fit(X, yn, w.kernel, w.length_scale, w.noise, slot=j)
        omega, phase = spectral_draw(w.kernel, features, w.d, rs)
        draws.append((omega, phase, rs.standard_normal((S, features)), rs.standard_normal((S, w.N)) * np.sqrt(w.noise)))

    def plain(fetch):
        return [eng.sample_paths(*draws[j], slot=j, y_mean=y_mean[j], y_std=y_std[j], return_values=fetch) for j in range(1 + C)]

    lb = np.full(C, -np.inf)
    ub = np.array([float(np.median(eng.sample_paths(*draws[j], slot=j, y_mean=y_mean[j], y_std=y_std[j], return_values=True)[2]))
                   for j in range(1, 1 + C)])
    t = {k: [] for k in ("constrained_ms", "host_rule_ms", "floor_ms")}

    def timed(key, fn, keep):
        t0 = time.perf_counter()
        out = fn()
        eng.synchronize()
        if keep:
            t[key].append((time.perf_counter() - t0) * 1e3)
        return out

    def today():
        return host_rule(np.array([p[2] for p in plain(True)]), lb, ub, y_std)

    feasible_share = None
    for r in range(warmup + runs):
        keep = r >= warmup
        got = timed("constrained_ms", lambda: eng.sample_paths_constrained(draws, lb, ub, y_mean, y_std), keep)
        want = timed("host_rule_ms", today, keep)
        timed("floor_ms", lambda: plain(False), keep)
        if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])):
            raise RuntimeError("the device's picks and the NumPy rule's on the fetched values differ")
        feasible_share = float(np.mean(got[3]))
    out = {k: stats(v) for k, v in t.items()}
    out["over_floor"] = out["constrained_ms"]["median"] / out["floor_ms"]["median"]
    out["host_rule_over_constrained"] = out["host_rule_ms"]["median"] / out["constrained_ms"]["median"]
    out["paths_with_a_feasible_candidate"] = feasible_share
    out["shape"] = {"N": w.N, "d": w.d, "M": w.M, "F": features, "paths": S, "constraints": C, "kernel": W.KERNEL_NAMES[w.kernel],
                    "length_scale": w.length_scale}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="C3")
    ap.add_argument("--constraints", default="1,2")
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrained_paths_bench.json"))
    args = ap.parse_args()
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs, "paths": S, "features": args.features,
                        "clock": "host perf_counter around the calls + stream synchronise"}}
    with GpEngine(0) as eng:
        out["device"] = eng.device_info().get("name")
        for C in (int(v) for v in args.constraints.split(",")):
            out[f"{args.shape}_constraints_{C}"] = measure(eng, W.ALL[args.shape], C, args.features, args.warmup, args.runs)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
