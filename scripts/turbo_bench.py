"""gpbo_generate_candidates_trust_region and suggest_turbo — the trust-region candidate generator next to the Philox generator that
writes the same bytes, one suggest_turbo call next to suggest_thompson, and a regret comparison of the two on Ackley-20.

    python scripts/turbo_bench.py [--warmup 3] [--runs 20] [--rounds 25] [--seeds 5] [--skip-regret] [--out FILE.json]

Protocol: everything in ONE process on ONE device; `warmup` untimed rounds, then the median of `runs` timed ones with
min / max beside it, the calls that are compared in alternation inside one loop.
  generator   M = 2^20, d = 16 and d = 64, p = 20 / d: KERNEL milliseconds from HIP events around the one launch
              (gpbo_debug_generate_ms, debug library — the same sources as the product) of the trust-region generator and of
              gpbo_generate_candidates over the same box, and the store floor 8 M d bytes over gpbo_hbm_copy_peak on this device.
  suggest     one suggest_turbo(q = 16, n_random = 2^20) and one suggest_thompson with the same arguments at N = 4096, d = 16
              (the C3 observations), theta held: host clock around the call (it ends synchronised).  The difference is MT19937
              jump-ahead generation against Sobol generation plus the host table build (sobol_tables, timed alone beside it).
  regret      the best value after `rounds` rounds of q = 8 on the negated 20-dimensional Ackley function over [-5, 10]^20 from
              2 d uniform points, `seeds` fixed seeds, n_random = 2^16, ARD Matern-2.5 with its theta search: suggest_turbo against
              suggest_thompson, and the lengths the trust region went through.
Prints one JSON object.
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


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def generator(eng, warmup, runs):
    from bayesianoptimization_amd.turbo import sobol_tables

    M = 1 << 20
    copy_gbps = float(np.median([eng.hbm_copy_peak(1 << 30) for _ in range(3)]))
    out = {"hbm_copy_peak_gbps": copy_gbps}
    for d in (16, 64):
        lo, hi = np.full(d, 0.2), np.full(d, 0.7)
        centre = np.full(d, 0.45)
        sv, shift = sobol_tables(d, 1)
        threshold = min(2 ** 32, int(20.0 / d * 2 ** 32))
        t = {"trust_region_ms": [], "philox_ms": []}
        for r in range(warmup + runs):
            eng.generate_candidates(M, lo, hi, 20240601 + r)
            a = eng.debug_generate_ms()
            eng.generate_candidates_trust_region(M, centre, lo, hi, sv, shift, 30, threshold, 77 + r)
            b = eng.debug_generate_ms()
            if r >= warmup:
                t["philox_ms"].append(a)
                t["trust_region_ms"].append(b)
        row = {k: stats(v) for k, v in t.items()}
        row["bytes"] = 8 * M * d
        row["perturb_probability"] = threshold / 2 ** 32
        row["store_floor_ms"] = 8 * M * d / (copy_gbps * 1e9) * 1e3
        out[f"M{M}_d{d}"] = row
    return out


class Optimizer:
    """What the suggest functions read of an accelerate()d BayesianOptimization."""

    def __init__(self, engine, X, y, bounds, kernel, seed, **gp_kw):
        from bayesianoptimization_amd import fused_acquisition as A
        from bayesianoptimization_amd.float_space import FloatSpace
        from bayesianoptimization_amd.gpr import HipGPR

        self._random_state = np.random.RandomState(seed)
        self._space = FloatSpace({f"x{j}": tuple(b) for j, b in enumerate(np.asarray(bounds, dtype=np.float64))})
        self._space.register_bulk(X, y)
        self._gp = HipGPR(kernel=kernel, alpha=1e-6, normalize_y=True, random_state=self._random_state, engine=engine, **gp_kw)
        self._acquisition_function = A.UpperConfidenceBound(kappa=2.576)


def suggest_calls(eng, warmup, runs):
    from sklearn.gaussian_process.kernels import Matern

    from bayesianoptimization_amd import TrustRegion, sobol_tables, suggest_thompson, suggest_turbo

    w = W.ALL["C3"]
    X, y, _ = W.make_observations(w)
    opt = Optimizer(eng, X, y, w.bounds_array(), Matern(nu=2.5, length_scale=w.length_scale), 5, optimizer=None)
    state = TrustRegion(w.d, 16)
    t = {"suggest_turbo_ms": [], "suggest_thompson_ms": [], "sobol_tables_ms": []}
    for r in range(warmup + runs):
        for key, fn in (("suggest_thompson_ms", lambda: suggest_thompson(opt, 16, n_random=w.M)),
                        ("suggest_turbo_ms", lambda: suggest_turbo(opt, 16, state, n_random=w.M)),
                        ("sobol_tables_ms", lambda: sobol_tables(w.d, r))):
            t0 = time.perf_counter()
            fn()
            eng.synchronize()
            if r >= warmup:
                t[key].append((time.perf_counter() - t0) * 1e3)
    out = {k: stats(v) for k, v in t.items()}
    out["shape"] = {"N": w.N, "d": w.d, "M": w.M, "q": 16, "n_features": 1024}
    return out


def ackley(x):
    x = np.asarray(x, dtype=np.float64)
    return float(-20.0 * np.exp(-0.2 * np.sqrt(np.mean(x * x))) - np.exp(np.mean(np.cos(2.0 * np.pi * x))) + 20.0 + np.e)


def regret(eng, rounds, seeds):
    from sklearn.gaussian_process.kernels import Matern

    from bayesianoptimization_amd import TrustRegion, suggest_thompson, suggest_turbo

    d, q, n_random = 20, 8, 1 << 16
    bounds = np.array([[-5.0, 10.0]] * d)
    out = {"turbo_best": [], "thompson_best": [], "turbo_lengths": [], "turbo_restarts": [], "initial_best": []}
    for seed in range(seeds):
        X = np.random.RandomState(1000 + seed).uniform(-5.0, 10.0, size=(2 * d, d))
        y = np.array([-ackley(x) for x in X])
        out["initial_best"].append(float(y.max()))
        for method in ("turbo", "thompson"):
            kernel = Matern(nu=2.5, length_scale=np.full(d, 5.0), length_scale_bounds=(0.05, 200.0))
            opt = Optimizer(eng, X.copy(), y.copy(), bounds, kernel, seed, n_restarts_optimizer=0)
            state, lengths = TrustRegion(d, q), []
            for _ in range(rounds):
                if method == "turbo":
                    picks = suggest_turbo(opt, q, state, n_random=n_random)
                    lengths.append(state.length)
                else:
                    picks = suggest_thompson(opt, q, n_random=n_random)
                for p in picks:
                    x = np.array(list(p.values()))
                    opt._space.register(x, -ackley(x))
            out[f"{method}_best"].append(float(opt._space.target.max()))
            if method == "turbo":
                out["turbo_lengths"].append(lengths)
                out["turbo_restarts"].append(state.restarts)
            print(f"# regret seed {seed} {method}: best {opt._space.target.max():.4f}", file=sys.stderr, flush=True)
    out["shape"] = {"d": d, "q": q, "rounds": rounds, "n_random": n_random, "initial_points": 2 * d, "function": "-Ackley on [-5, 10]^20"}
    out["turbo_mean"] = float(np.mean(out["turbo_best"]))
    out["thompson_mean"] = float(np.mean(out["thompson_best"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--skip-regret", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs,
                        "clock": "generator: HIP events around the kernel; suggest: host perf_counter around call + stream synchronise"}}
    with GpEngine(0, debug=True) as eng:
        info = eng.device_info()
        out["device"] = {"name": info.get("name") or info.get("arch"), "arch": info.get("arch"), "compute_units": info.get("compute_units")}
        out["generator"] = generator(eng, args.warmup, args.runs)
        print("# generator done", file=sys.stderr, flush=True)
        out["suggest"] = suggest_calls(eng, args.warmup, max(3, args.runs // 4))
        print("# suggest done", file=sys.stderr, flush=True)
        if not args.skip_regret:
            out["regret"] = regret(eng, args.rounds, args.seeds)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
