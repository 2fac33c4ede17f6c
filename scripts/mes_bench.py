"""gpbo_mes_argbest — max-value entropy search values over the resident candidates and their arg-best — next to gpbo_acq_argbest
with EI on the same resident posterior, and the whole suggest_mes call next to suggest_thompson(q = 16, refine = 4), at the C3 shape
of BASELINE.json (N = 4096, d = 16, M = 2^20).

    python scripts/mes_bench.py [--shapes C3] [--samples 1,16,64] [--features 1024] [--warmup 3] [--runs 10] [--out FILE.json]

Protocol: random data (workloads.make_observations, candidates from the device generator), ONE process, ONE device,
ONE posterior pass left resident; `warmup` untimed rounds, then the median of `runs` timed ones with min / max beside it, the timed
calls in alternation inside one loop.  Two clocks per call: a host clock around the call (it ends in a stream synchronise: the
fetch of the selection's records), and the library's own event pair around the value kernel + the selection launches
(`last_timings()["acq_argbest"]`, both entry points record the same pair).  Per round: EI arg-best -> MES with S sampled maxima for
every S of --samples, y* spread above the best observation as a draw's maximum is (gamma > 0 for nearly every candidate: the
complement branch alone) -> MES with S = 16 and y* spread over the posterior means' own range (gamma of both signs inside most
waves: every branch, the divergent case).  All with k_seeds = 0 and again with k_seeds = 10.  `per_sample_us` = the slope of the
kernel-side time over S between the smallest and the largest S.
Then, at fixed theta (optimizer=None: the acquisition's own cost, no theta search), on an optimizer stand-in: suggest_mes(n_samples
= 16, refine = 4) and suggest_thompson(q = 16, refine = 4) over n_random = M candidates, alternated.  suggest_mes = suggest_thompson's
engine calls + one posterior pass + gpbo_mes_argbest.  Prints one JSON object.
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
from bayesianoptimization_amd import suggest_mes, suggest_thompson  # noqa: E402
from bayesianoptimization_amd import workloads as W  # noqa: E402
from bayesianoptimization_amd.engine import GpEngine  # noqa: E402
from bayesianoptimization_amd.float_space import FloatSpace  # noqa: E402
from bayesianoptimization_amd.gpr import HipGPR  # noqa: E402

EI = 1


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


class Optimizer:
    """what suggest_mes / suggest_thompson read of an accelerate()d BayesianOptimization, at FIXED theta (optimizer=None)"""

    def __init__(self, eng, w, X, y):
        from sklearn.gaussian_process.kernels import Matern

        self._random_state = np.random.RandomState(7)
        self._space = FloatSpace(w.pbounds())
        self._space.register_bulk(X, y)
        self._gp = HipGPR(kernel=Matern(nu=2.5, length_scale=w.length_scale), alpha=w.noise, normalize_y=True, optimizer=None,
                          random_state=self._random_state, engine=eng)
        self._acquisition_function = A.UpperConfidenceBound(kappa=2.576)


def measure(eng, w, samples, features, warmup, runs):
    X, y, _ = W.make_observations(w)
    yn, ym, ys = W.normalize_targets(y)
    b = w.bounds_array()
    eng.generate_candidates(w.M, np.ascontiguousarray(b[:, 0]), np.ascontiguousarray(b[:, 1]), 20240601)
    eng.fit(X, yn, w.kernel, w.length_scale, w.noise)
    mu, sd = eng.posterior(0, ym, ys)
    y_max = float(y.max())
    rs = np.random.RandomState(11)
    above = {S: y_max + np.abs(rs.standard_normal(S)) * 0.5 * ys for S in samples}
    mixed = rs.uniform(np.quantile(mu, 0.05), np.quantile(mu, 0.95), 16)
    g = (mixed[None, :] - mu[:4096, None]) / sd[:4096, None]
    calls = {"ei": lambda k: eng.acq_argbest(EI, 0.01, y_max, k_seeds=k)}
    for S in samples:
        calls[f"mes_s{S}"] = lambda k, S=S: eng.mes_argbest(above[S], k_seeds=k)
    calls["mes_s16_mixed_ranges"] = lambda k: eng.mes_argbest(mixed, k_seeds=k)
    out = {}
    for k in (0, 10):
        host = {n: [] for n in calls}
        dev = {n: [] for n in calls}
        for r in range(warmup + runs):
            for n, fn in calls.items():
                eng.synchronize()
                t0 = time.perf_counter()
                fn(k)
                eng.synchronize()
                t1 = time.perf_counter()
                if r >= warmup:
                    host[n].append((t1 - t0) * 1e3)
                    dev[n].append(eng.last_timings()["acq_argbest"])
        res = {n: {"call_ms": stats(host[n]), "kernels_ms": stats(dev[n])} for n in calls}
        lo, hi = min(samples), max(samples)
        if hi > lo:
            res["per_sample_us"] = 1e3 * (res[f"mes_s{hi}"]["kernels_ms"]["median"] - res[f"mes_s{lo}"]["kernels_ms"]["median"]) / (hi - lo)
        for S in samples:
            res[f"mes_s{S}_over_ei"] = res[f"mes_s{S}"]["kernels_ms"]["median"] / res["ei"]["kernels_ms"]["median"]
        out[f"k_seeds_{k}"] = res
    out["gamma_share_positive"] = {"above": float(((above[max(samples)][None, :] - mu[:4096, None]) > 0).mean()),
                                   "mixed": float((g > 0).mean()), "mixed_below_minus_1": float((g <= -1).mean())}
    # the whole calls, at fixed theta
    opt = Optimizer(eng, w, X, y)
    mes_ms, ts_ms = [], []
    for r in range(warmup + runs):
        eng.synchronize()
        t0 = time.perf_counter()
        params, info = suggest_mes(opt, 16, n_random=w.M, n_features=features, refine=4, return_info=True)
        eng.synchronize()
        t1 = time.perf_counter()
        picks = suggest_thompson(opt, 16, n_random=w.M, n_features=features, refine=4)
        eng.synchronize()
        t2 = time.perf_counter()
        if len(picks) != 16 or len(params) != w.d:
            raise RuntimeError("a driver returned the wrong number of picks")
        if r >= warmup:
            mes_ms.append((t1 - t0) * 1e3)
            ts_ms.append((t2 - t1) * 1e3)
    out["suggest_mes_s16_refine4_ms"] = stats(mes_ms)
    out["suggest_thompson_q16_refine4_ms"] = stats(ts_ms)
    out["suggest_mes_over_suggest_thompson"] = out["suggest_mes_s16_refine4_ms"]["median"] / out["suggest_thompson_q16_refine4_ms"]["median"]
    out["last_y_star_above_best_observation_y_std"] = ((info["y_star"] - y_max) / ys).tolist()
    out["shape"] = {"N": w.N, "d": w.d, "M": w.M, "F": features, "kernel": W.KERNEL_NAMES[w.kernel], "length_scale": w.length_scale}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C3")
    ap.add_argument("--samples", default="1,16,64")
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    samples = [int(s) for s in args.samples.split(",")]
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs, "samples": samples, "features": args.features,
                        "clock": "call_ms: host perf_counter around call + stream synchronise; kernels_ms: the library's event pair "
                                 "around the value kernel and the selection launches"}}
    with GpEngine(0) as eng:
        out["device"] = eng.device_info().get("name")
        for name in args.shapes.split(","):
            out[name] = measure(eng, W.ALL[name], samples, args.features, args.warmup, args.runs)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
