"""gpbo_kg_argbest — knowledge-gradient values over the resident candidates and their arg-best — stage by stage, next to the full
gpbo_posterior of the same box and to gpbo_sample_paths with 16 paths and ONE feature (the yardstick for one 16-column pass over
the training points), at N = 4096, d = 16, M = 2^20 (the C3 shape of BASELINE.json) and J = 16 / 32 / 64 reference points.

    python scripts/kg_bench.py [--shape C3] [--points 16,32,64] [--warmup 3] [--runs 10] [--out FILE.json]

Protocol: random data (workloads.make_observations, candidates from the device generator), `warmup` untimed rounds,
then the median of `runs` timed ones with min / max beside it; everything in ONE process on ONE device, all timed calls in alternation
inside one loop.  The three stages of a kg_argbest call (points: k*, means and solves | covariances | envelopes) are KERNEL times
from HIP events around them (gpbo_debug_kg_stage_ms, debug library — the same sources as the product); the call itself, the
posterior pass and sample_paths are host clocks around a call that ends in a stream synchronise.  Per J the covariance kernel runs
with every accumulator count that serves it (GPBO_KG_NS = 16 | 32 | 64 columns per pass, the debug library's switch): the numbers
the dispatch rule of kg.hip (kg_cov_ns) rests on.  Prints one JSON object.
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
from bayesianoptimization_amd.engine import UCB, GpEngine  # noqa: E402
from bayesianoptimization_amd.thompson import spectral_draw  # noqa: E402


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def measure(eng, w, points, warmup, runs):
    X, y, _ = W.make_observations(w)
    yn, ym, ys = W.normalize_targets(y)
    b = w.bounds_array()
    eng.generate_candidates(w.M, b[:, 0], b[:, 1], 20240601)
    rs = np.random.RandomState(11)
    omega, phase = spectral_draw(w.kernel, 1, w.d, rs)
    weights = rs.standard_normal((16, 1))
    eps = rs.standard_normal((16, w.N)) * np.sqrt(w.noise)
    eng.fit(X, yn, w.kernel, w.length_scale, w.noise)
    eng.posterior(0, ym, ys, fetch=False)
    top = eng.acq_argbest(UCB, 0.0, k_seeds=32)[2]
    idx = np.concatenate([top, np.setdiff1d(np.arange(128), top)[:32]]).astype(np.int64)
    pts_all = np.asarray(eng.get_candidate_rows(idx, w.d), dtype=np.float64)
    variants = [(J, ns) for J in points for ns in (16, 32, 64) if ns == 16 or ns < 2 * J]
    t = {"full_posterior_ms": [], "sample_paths_16_one_feature_ms": []}
    for J, ns in variants:
        for k in ("call_ms", "points_ms", "cov_ms", "envelope_ms"):
            t[f"J{J}_ns{ns}_{k}"] = []
    picks = {}
    for r in range(warmup + runs):
        keep = r >= warmup

        def timed(key, fn):
            t0 = time.perf_counter()
            out = fn()
            eng.synchronize()
            if keep:
                t[key].append((time.perf_counter() - t0) * 1e3)
            return out

        timed("full_posterior_ms", lambda: eng.posterior(0, ym, ys, fetch=False))
        timed("sample_paths_16_one_feature_ms", lambda: eng.sample_paths(omega, phase, weights, eps, y_mean=ym, y_std=ys))
        for J, ns in variants:
            os.environ["GPBO_KG_NS"] = str(ns)
            pts = np.concatenate([pts_all[:(J + 1) // 2], pts_all[32:32 + J // 2]])
            best = timed(f"J{J}_ns{ns}_call_ms", lambda: eng.kg_argbest(pts, y_mean=ym, y_std=ys))[0]
            ms = eng.debug_kg_stage_ms()
            if keep:
                for k, v in zip(("points_ms", "cov_ms", "envelope_ms"), ms):
                    t[f"J{J}_ns{ns}_{k}"].append(v)
            if picks.setdefault(J, best) != best:
                raise RuntimeError("kg_argbest's pick depends on the accumulator count or the run")
    os.environ.pop("GPBO_KG_NS", None)
    out = {k: stats(v) for k, v in t.items()}
    out["picks"] = {str(J): int(v) for J, v in picks.items()}
    out["shape"] = {"N": w.N, "d": w.d, "M": w.M, "kernel": W.KERNEL_NAMES[w.kernel], "length_scale": w.length_scale,
                    "noise": w.noise}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="C3")
    ap.add_argument("--points", default="16,32,64")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs,
                        "clock": "stages: HIP events around the kernels; calls: host perf_counter around call + stream synchronise"}}
    with GpEngine(0, debug=True) as eng:
        info = eng.device_info()
        out["device"] = {"name": info.get("name") or info.get("arch"), "arch": info.get("arch"), "compute_units": info.get("compute_units")}
        out[args.shape] = measure(eng, W.ALL[args.shape], [int(v) for v in args.points.split(",")], args.warmup, args.runs)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
