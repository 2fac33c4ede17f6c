"""gpiv_ivr_argbest — integrated posterior variance reduction over the resident candidates and its arg-best — stage by stage, next to
the full gpbo_posterior of the same box and, at J = 64 (the only shape both serve), to gpbo_kg_argbest's covariance kernel, at
N = 4096, d = 16, M = 2^20 (the C3 shape of BASELINE.json) and J = 64 / 256 / 1024 / 4096 integration points.

    python scripts/ivr_bench.py [--shape C3] [--points 64,256,1024,4096] [--warmup 2] [--runs 5] [--out profiles/ivr_bench.json]

Protocol: random data (workloads.make_observations, candidates from the device generator), `warmup` untimed rounds,
then the median of `runs` timed ones with min / max beside it; everything in ONE process on ONE device, all timed calls in alternation
inside one loop.  The three stages of an ivr_argbest call (points: k*, solves and packing | scores | selection) are KERNEL times
from HIP events around them (gpiv_debug_stage_ms, debug library — the same sources as the product); so is kg_cov_kernel's
(gpbo_debug_kg_stage_ms); the calls themselves and the posterior pass are host clocks around a call that ends in a stream
synchronise.  The score kernel's rate is the product's 2 M N J flops (the operations the algorithm needs; the padding of J and N,
the regeneration of k* per tile and the kernel values themselves are not counted) over its kernel time, next to gpbo_mfma_f64_peak
measured in the same process before and after the loop.  Prints one JSON object.
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


def measure(eng, w, points, warmup, runs):
    X, y, _ = W.make_observations(w)
    yn, ym, ys = W.normalize_targets(y)
    b = w.bounds_array()
    eng.generate_candidates(w.M, b[:, 0], b[:, 1], 20240601)
    eng.fit(X, yn, w.kernel, w.length_scale, w.noise)
    eng.posterior(0, ym, ys, fetch=False)
    pts_all = np.asarray(eng.get_candidate_rows(np.arange(max(points), dtype=np.int64), w.d), dtype=np.float64)
    peak = [eng.mfma_f64_peak()]
    t = {"full_posterior_ms": [], "kg_J64_call_ms": [], "kg_J64_cov_ms": []}
    for J in points:
        for k in ("call_ms", "points_ms", "score_ms", "select_ms"):
            t[f"J{J}_{k}"] = []
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
        timed("kg_J64_call_ms", lambda: eng.kg_argbest(pts_all[:64], y_mean=ym, y_std=ys))
        if keep:
            t["kg_J64_cov_ms"].append(eng.debug_kg_stage_ms()[1])
        for J in points:
            best = timed(f"J{J}_call_ms", lambda: eng.ivr_argbest(pts_all[:J], y_mean=ym, y_std=ys))[0]
            ms = eng.debug_ivr_stage_ms()
            if keep:
                for k, v in zip(("points_ms", "score_ms", "select_ms"), ms):
                    t[f"J{J}_{k}"].append(v)
            if picks.setdefault(J, best) != best:
                raise RuntimeError("ivr_argbest's pick depends on the run")
    peak.append(eng.mfma_f64_peak())
    out = {k: stats(v) for k, v in t.items()}
    out["mfma_f64_peak_tflops"] = {"before": peak[0], "after": peak[1]}
    for J in points:
        tflops = 2.0 * w.M * w.N * J / (out[f"J{J}_score_ms"]["median"] * 1e-3) / 1e12
        out[f"J{J}_score_tflops"] = tflops
        out[f"J{J}_score_share_of_mfma_peak"] = tflops / min(peak)
    out["picks"] = {str(J): int(v) for J, v in picks.items()}
    out["shape"] = {"N": w.N, "d": w.d, "M": w.M, "kernel": W.KERNEL_NAMES[w.kernel], "length_scale": w.length_scale,
                    "noise": w.noise}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="C3")
    ap.add_argument("--points", default="64,256,1024,4096")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivr_bench.json"))
    args = ap.parse_args()
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs,
                        "clock": "stages: HIP events around the kernels; calls: host perf_counter around call + stream synchronise",
                        "flops": "2 M N J per score kernel, padding and kernel values not counted"}}
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
