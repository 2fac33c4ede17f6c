"""The theta search of a scaled model  C * Matern(2.5) + WhiteKernel  with its restarts one after another (gpbo_lml_scaled) against
side by side in lanes (gpbo_lml_batch_scaled), and one six-lane scaled round beside one six-lane unit round (gpbo_lml_batch).

    python scripts/scaled_lanes_timing.py [--sizes 64,256,512,2048] [--repeats 7] [--out FILE.json]

One child process per reading (a size of the search, a size of the round), so that no reading inherits another's warmed pools; inside
a reading the two modes alternate after three warm-ups each, so that a drift of the clocks lands on both alike.  Per mode the median
wall time with min and max; a fit and a round both end in a stream synchronisation.  The search: HipGPR.fit, 5 restarts, one
length scale per dimension at d = 8 (10 free hyper-parameters), the same RandomState seed for both modes — the same iterates, so
the same number of evaluations.  Prints one JSON object.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, ALPHA, WARMUPS = 8, 1e-6, 3


def data(N):
    rng = np.random.RandomState(N)
    X = rng.uniform(size=(N, D))
    return X, np.sin(3.0 * X.sum(1)) + 0.1 * rng.standard_normal(N)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def search_reading(N, repeats):
    from sklearn.gaussian_process.kernels import ConstantKernel, Matern, WhiteKernel

    from bayesianoptimization_amd.engine import GpEngine
    from bayesianoptimization_amd.gpr import HipGPR

    X, y = data(N)
    kernel = ConstantKernel(1.0) * Matern(nu=2.5, length_scale=np.ones(D)) + WhiteKernel(1e-2)
    ms = {False: [], True: []}
    found = {}
    with GpEngine(0) as eng:
        eng.set_timing(False)
        for it in range(WARMUPS + repeats):
            for lanes in (False, True):
                gp = HipGPR(kernel=kernel, alpha=ALPHA, normalize_y=True, n_restarts_optimizer=5, engine=eng,
                            random_state=np.random.RandomState(0), scaled_kernels=True, scaled_lanes=lanes)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    t0 = time.perf_counter()
                    gp.fit(X, y)
                    t = (time.perf_counter() - t0) * 1e3
                if it >= WARMUPS:
                    ms[lanes].append(t)
                found[lanes] = (gp.kernel_.theta.copy(), float(gp.log_marginal_likelihood_value_))
                if lanes:
                    rounds, evals = int(gp.theta_search_rounds_), int(gp.theta_search_evals_)
        device = eng.device_info().get("name")
    same = bool(np.array_equal(found[False][0], found[True][0]) and found[False][1] == found[True][1])
    off, on = stats(ms[False]), stats(ms[True])
    return {"N": N, "d": D, "device": device, "fit_ms_sequential": off, "fit_ms_lanes": on, "ratio_of_medians": off["median"] / on["median"],
            "lockstep_rounds": rounds, "evaluations": evals, "same_theta_and_value": same}


def round_reading(N, repeats):
    from bayesianoptimization_amd.engine import MATERN25, GpEngine

    X, y = data(N)
    yn = (y - y.mean()) / y.std()
    rng = np.random.RandomState(1)
    ls = np.ascontiguousarray(rng.uniform(0.5, 1.5, size=(6, D)))
    c, w = np.geomspace(0.3, 40.0, 6), np.array([2e-3, 0.0, 5e-2, 1e-4, 0.3, 7e-3])
    ms = {"unit": [], "scaled": []}
    with GpEngine(0) as eng:
        eng.set_timing(False)
        eng.lml_batch_arrays(X, yn, MATERN25, ls, ALPHA)        # the resident inputs, shared by both forms
        for it in range(WARMUPS + repeats):
            for form in ("unit", "scaled"):
                t0 = time.perf_counter()
                if form == "unit":
                    eng.lml_batch_arrays(X, yn, MATERN25, ls, ALPHA, True, True)
                else:
                    eng.lml_batch_scaled_arrays(X, yn, MATERN25, ls, c, w, ALPHA, True, True)
                t = (time.perf_counter() - t0) * 1e3
                if it >= WARMUPS:
                    ms[form].append(t)
        device = eng.device_info().get("name")
    unit, scaled = stats(ms["unit"]), stats(ms["scaled"])
    return {"N": N, "d": D, "lanes": 6, "device": device, "unit_round_ms": unit, "scaled_round_ms": scaled,
            "extra_ms_of_medians": scaled["median"] - unit["median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256,512,2048")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reading", default=None, help="(child) search or round")
    ap.add_argument("--N", type=int, default=0, help="(child) the size of the reading")
    args = ap.parse_args()
    if args.reading:
        fn = search_reading if args.reading == "search" else round_reading
        print(json.dumps(fn(args.N, args.repeats if args.reading == "search" else 30 * args.repeats)))
        return
    out = {"what": "C * Matern(2.5) + WhiteKernel, d = 8, one length scale per dimension, 5 restarts; wall ms", "warmups": WARMUPS,
           "theta_search": [], "six_lane_round": []}
    for N in [int(s) for s in args.sizes.split(",")]:
        for reading, key in (("search", "theta_search"), ("round", "six_lane_round")):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reading", reading, "--N", str(N), "--repeats", str(args.repeats)],
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.stderr.write(r.stderr)
                raise SystemExit(f"the {reading} reading at N = {N} failed (exit status {r.returncode})")
            out[key].append(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
