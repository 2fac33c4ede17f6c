"""gpje_jes_argbest — joint entropy search over the resident candidates and its arg-best — stage by stage, next to
gpiv_ivr_argbest at J = 64, gpbo_kg_argbest at J = 16 / 64 and the full gpbo_posterior of the same box, at N = 4096, d = 16,
M = 2^20 (the C3 shape of BASELINE.json) and S = 16 / 32 / 64 sampled optima (one per split of csrc/jes_plan.h).

    python scripts/jes_bench.py [--shape C3] [--samples 16,32,64] [--warmup 2] [--runs 5] [--out profiles/jes_bench.json]

Protocol: random data (workloads.make_observations, candidates from the device generator), `warmup` untimed rounds,
then the median of `runs` timed ones with min / max beside it; everything in ONE process on ONE device, all timed calls in alternation
inside one loop.  The sampled optima are the first S candidate rows with f* = mu + 2 sd there (a maximum two posterior deviations
above its own mean, so that beta takes both signs over the candidates).  The three stages of a jes_argbest call (points: k*, solves,
m_s / p_s and packing | scores | selection) are KERNEL times from HIP events around them (gpje_debug_stage_ms, debug library — the
same sources as the product); so are gpiv_ivr_argbest's (gpiv_debug_stage_ms) and kg_cov_kernel's (gpbo_debug_kg_stage_ms); the calls
themselves and the posterior pass are host clocks around a call that ends in a stream synchronise.  Prints one JSON object.
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


def measure(eng, w, samples, warmup, runs):
    X, y, _ = W.make_observations(w)
    yn, ym, ys = W.normalize_targets(y)
    b = w.bounds_array()
    eng.generate_candidates(w.M, b[:, 0], b[:, 1], 20240601)
    eng.fit(X, yn, w.kernel, w.length_scale, w.noise)
    mu, sd = eng.posterior(0, ym, ys)
    pts = np.asarray(eng.get_candidate_rows(np.arange(64, dtype=np.int64), w.d), dtype=np.float64)
    f_star = mu[:64] + 2.0 * sd[:64]
    t = {"full_posterior_ms": [], "ivr_J64_score_ms": []}
    for J in (16, 64):
        t[f"kg_J{J}_cov_ms"] = []
    for S in samples:
        for k in ("call_ms", "points_ms", "score_ms", "select_ms"):
            t[f"S{S}_{k}"] = []
    picks = {}
    for r in range(warmup + runs):
        keep = r >= warmup

        def timed(key, fn):
            t0 = time.perf_counter()
            out = fn()
            eng.synchronize()
            if keep and key:
                t[key].append((time.perf_counter() - t0) * 1e3)
            return out

        timed("full_posterior_ms", lambda: eng.posterior(0, ym, ys, fetch=False))
        for J in (16, 64):
            eng.kg_argbest(pts[:J], y_mean=ym, y_std=ys)
            if keep:
                t[f"kg_J{J}_cov_ms"].append(eng.debug_kg_stage_ms()[1])
        eng.ivr_argbest(pts, y_mean=ym, y_std=ys)
        if keep:
            t["ivr_J64_score_ms"].append(eng.debug_ivr_stage_ms()[1])
        for S in samples:
            best = timed(f"S{S}_call_ms", lambda: eng.jes_argbest(pts[:S], f_star[:S], y_mean=ym, y_std=ys))[0]
            ms = eng.debug_jes_stage_ms()
            if keep:
                for k, v in zip(("points_ms", "score_ms", "select_ms"), ms):
                    t[f"S{S}_{k}"].append(v)
            if picks.setdefault(S, best) != best:
                raise RuntimeError("jes_argbest's pick depends on the run")
    out = {k: stats(v) for k, v in t.items()}
    out["picks"] = {str(S): int(v) for S, v in picks.items()}
    out["shape"] = {"N": w.N, "d": w.d, "M": w.M, "kernel": W.KERNEL_NAMES[w.kernel], "length_scale": w.length_scale,
                    "noise": w.noise}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="C3")
    ap.add_argument("--samples", default="16,32,64")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jes_bench.json"))
    args = ap.parse_args()
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs,
                        "clock": "stages: HIP events around the kernels; calls: host perf_counter around call + stream synchronise"}}
    with GpEngine(0, debug=True) as eng:
        info = eng.device_info()
        out["device"] = {"name": info.get("name") or info.get("arch"), "arch": info.get("arch"), "compute_units": info.get("compute_units")}
        out[args.shape] = measure(eng, W.ALL[args.shape], [int(v) for v in args.samples.split(",")], args.warmup, args.runs)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
