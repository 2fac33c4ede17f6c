"""gpls_sur_argbest — SUR for an excursion set over the resident candidates — stage by stage next to gpiv_ivr_argbest, which runs
the same covariance product with a trivial epilogue, at N = 4096, d = 16, M = 2^20 (the C3 shape of BASELINE.json) and J = 64 / 256 /
1024 integration points.

    python scripts/sur_bench.py [--shape C3] [--points 64,256,1024] [--warmup 2] [--runs 5] [--out profiles/sur_bench.json]

Protocol, as scripts/ivr_bench.py: random data, `warmup` untimed rounds, then the median of `runs` timed ones with
min / max beside it; ONE process, ONE device, both calls in alternation inside one loop.  The stages (points | scores | selection) are
KERNEL times from HIP events (gpls_debug_stage_ms, gpiv_debug_stage_ms; debug library — the same sources as the product).  Per J the
two score kernels and their ratio; the SUR epilogue's cost per (candidate, point) pair is the difference of the two over M J.  The
level is the targets' median, so that the points' h_j are spread around 0.  Prints one JSON object.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bayesianoptimization_amd import workloads as W  # noqa: E402
from bayesianoptimization_amd.engine import GpEngine  # noqa: E402

STAGES = ("points_ms", "score_ms", "select_ms")


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
    level = float(np.median(y))
    t = {f"J{J}_{which}_{k}": [] for J in points for which in ("sur", "ivr") for k in STAGES}
    picks = {}
    for r in range(warmup + runs):
        for J in points:
            best = eng.sur_argbest(pts_all[:J], level, y_mean=ym, y_std=ys)[0]
            sur_ms = eng.debug_sur_stage_ms()
            eng.ivr_argbest(pts_all[:J], y_mean=ym, y_std=ys)
            ivr_ms = eng.debug_ivr_stage_ms()
            if r >= warmup:
                for which, ms in (("sur", sur_ms), ("ivr", ivr_ms)):
                    for k, v in zip(STAGES, ms):
                        t[f"J{J}_{which}_{k}"].append(v)
            if picks.setdefault(J, best) != best:
                raise RuntimeError("sur_argbest's pick depends on the run")
    out = {k: stats(v) for k, v in t.items()}
    for J in points:
        sur, ivr = out[f"J{J}_sur_score_ms"]["median"], out[f"J{J}_ivr_score_ms"]["median"]
        out[f"J{J}_score_ratio_sur_over_ivr"] = sur / ivr
        out[f"J{J}_epilogue_ns_per_pair"] = (sur - ivr) * 1e6 / (w.M * float(J))
        out[f"J{J}_sur_pairs_per_s"] = w.M * float(J) / (sur * 1e-3)
    out["picks"] = {str(J): int(v) for J, v in picks.items()}
    out["level"] = level
    out["shape"] = {"N": w.N, "d": w.d, "M": w.M, "kernel": W.KERNEL_NAMES[w.kernel], "length_scale": w.length_scale,
                    "noise": w.noise}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="C3")
    ap.add_argument("--points", default="64,256,1024")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sur_bench.json"))
    args = ap.parse_args()
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs, "clock": "stages: HIP events around the kernels",
                        "yardstick": "gpiv_ivr_argbest's score kernel: the same product, a squared weighted row sum behind it"}}
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
