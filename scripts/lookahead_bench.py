"""gpla_ei2_argbest — two-step lookahead EI over the resident candidates and its arg-best — stage by stage, next to gpje_jes_argbest's
score kernel at the same column count and the full gpbo_posterior of the same box, at N = 4096, d = 16, M = 2^20 (the C3 shape of
BASELINE.json) and (J, H) = (16, 8), (32, 8), (64, 16), (64, 32) reference points and Gauss-Hermite nodes.

    python scripts/lookahead_bench.py [--shape C3] [--cases 16x8,32x8,64x16,64x32] [--warmup 2] [--runs 5] [--out profiles/lookahead_bench.json]

Protocol: random data (workloads.make_observations, candidates from the device generator), `warmup` untimed rounds,
then the median of `runs` timed ones with min / max beside it; everything in ONE process on ONE device, all timed calls in alternation
inside one loop.  The reference points are the first J candidate rows, y_best the largest observed target.  The three stages of an
ei2_argbest call (points | scores | selection) are KERNEL times from HIP events around them (gpla_debug_stage_ms, debug library — the
same sources as the product); so are gpje_jes_argbest's (gpje_debug_stage_ms), called with S = J sampled optima at the same rows; the
calls themselves and the posterior pass are host clocks around a call that ends in a stream synchronise.  The two score kernels run
the SAME product (csrc/jes_product.h), so their difference is the epilogues': reported per case as `epilogue_minus_jes_ms`, and the
lookahead epilogue's H (J + 1) M evaluations of E[(Y - a)^+] per second of that difference as `g_evals_per_s_over_difference` (a
LOWER bound on the time per evaluation, since JES's own epilogue is inside its kernel) and per second of the whole score kernel as
`g_evals_per_s_over_kernel`.  Prints one JSON object.
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


def measure(eng, w, cases, warmup, runs):
    X, y, _ = W.make_observations(w)
    yn, ym, ys = W.normalize_targets(y)
    b = w.bounds_array()
    eng.generate_candidates(w.M, b[:, 0], b[:, 1], 20240601)
    eng.fit(X, yn, w.kernel, w.length_scale, w.noise)
    mu, sd = eng.posterior(0, ym, ys)
    pts = np.asarray(eng.get_candidate_rows(np.arange(64, dtype=np.int64), w.d), dtype=np.float64)
    f_star = mu[:64] + 2.0 * sd[:64]
    y_best = float(np.max(y))
    t = {"full_posterior_ms": []}
    for J in sorted({J for J, _ in cases}):
        t[f"jes_S{J}_score_ms"] = []
    for J, H in cases:
        for k in ("call_ms", "points_ms", "score_ms", "select_ms"):
            t[f"J{J}_H{H}_{k}"] = []
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
        for J in sorted({J for J, _ in cases}):
            eng.jes_argbest(pts[:J], f_star[:J], y_mean=ym, y_std=ys)
            if keep:
                t[f"jes_S{J}_score_ms"].append(eng.debug_jes_stage_ms()[1])
        for J, H in cases:
            nodes, weights = np.polynomial.hermite_e.hermegauss(H)
            weights = weights / np.sqrt(2.0 * np.pi)
            best = timed(f"J{J}_H{H}_call_ms", lambda: eng.ei2_argbest(pts[:J], nodes, weights, y_best, y_mean=ym, y_std=ys))[0]
            ms = eng.debug_ei2_stage_ms()
            if keep:
                for k, v in zip(("points_ms", "score_ms", "select_ms"), ms):
                    t[f"J{J}_H{H}_{k}"].append(v)
            if picks.setdefault((J, H), best) != best:
                raise RuntimeError("ei2_argbest's pick depends on the run")
    out = {k: stats(v) for k, v in t.items()}
    for J, H in cases:
        score, jes = out[f"J{J}_H{H}_score_ms"]["median"], out[f"jes_S{J}_score_ms"]["median"]
        evals = float(H) * (J + 1) * w.M
        out[f"J{J}_H{H}_epilogue"] = {"epilogue_minus_jes_ms": score - jes, "score_over_jes": score / jes,
                                      "g_evals_per_s_over_difference": evals / ((score - jes) * 1e-3) if score > jes else None,
                                      "g_evals_per_s_over_kernel": evals / (score * 1e-3)}
    out["picks"] = {f"{J}x{H}": int(v) for (J, H), v in picks.items()}
    out["shape"] = {"N": w.N, "d": w.d, "M": w.M, "kernel": W.KERNEL_NAMES[w.kernel], "length_scale": w.length_scale,
                    "noise": w.noise}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="C3")
    ap.add_argument("--cases", default="16x8,32x8,64x16,64x32")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookahead_bench.json"))
    args = ap.parse_args()
    cases = [tuple(int(v) for v in c.split("x")) for c in args.cases.split(",")]
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs,
                        "clock": "stages: HIP events around the kernels; calls: host perf_counter around call + stream synchronise"}}
    with GpEngine(0, debug=True) as eng:
        info = eng.device_info()
        out["device"] = {"name": info.get("name") or info.get("arch"), "arch": info.get("arch"), "compute_units": info.get("compute_units")}
        out[args.shape] = measure(eng, W.ALL[args.shape], cases, args.warmup, args.runs)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
