"""gppf_pfes_argbest — Pareto-frontier entropy search over the resident candidates and its arg-best — stage by stage, next to its two
multi-objective siblings in the same process: gpbo_ehvi_argbest's value kernel over the observed front, and ONE greedy step of
gpbo_qnhvi_greedy (qnehvi_score_kernel, selection and front update) over the same number of draws; at N = 4096, d = 16, M = 2^20 (the
C3 shape of BASELINE.json) with S = 16 and 64 sampled fronts.

    python scripts/pfes_bench.py [--shape C3] [--samples 16,64] [--warmup 2] [--runs 5] [--out profiles/pfes_bench.json]

Protocol: random data (workloads.make_observations and a second target column, candidates from the device generator),
`warmup` untimed rounds, then the median of `runs` timed ones with min / max beside it; everything in ONE process on ONE device, all
timed calls in alternation inside one loop.  The fronts are built on the device from S joint draws (F = 1024 features) at the first
16384 candidates.  The three stages of a pfes_argbest call (draws + fronts | scores | selection) are KERNEL times from HIP events
around them (gppf_debug_stage_ms, debug library — the same sources as the product); so are the siblings' (gpbo_debug_ehvi_ms;
gpbo_debug_qnehvi_stage_ms of a q = 1 call, whose third stage is one step); the calls themselves and the posterior passes are host
clocks around a call that ends in a stream synchronise.  `strip_evals_per_s` is M * sum_s n_s — each one new level per objective:
one erfc, one exp and one division each — over the score stage.  Prints one JSON object.
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
from bayesianoptimization_amd.multiobjective import box_decomposition, pareto_front  # noqa: E402
from bayesianoptimization_amd.thompson import spectral_draw  # noqa: E402

FEATURES = 1024
PATH_NOISE = 1e-2      # the noise the draws' eps are scaled with (normalised-target units)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def make_draws(w, G, S, rs):
    return [[spectral_draw(w.kernel, FEATURES, w.d, rs) + (rs.standard_normal((S, FEATURES)), rs.standard_normal((S, w.N)) * np.sqrt(PATH_NOISE))
             for _ in range(G)] for _ in range(2)]


def measure(eng, w, samples, warmup, runs):
    X, y0, _ = W.make_observations(w)
    y1 = np.cos(3.0 * X.sum(1) + 0.7) + 0.1 * np.random.RandomState(5).standard_normal(w.N)
    norm = [W.normalize_targets(y) for y in (y0, y1)]
    y_mean, y_std = [n[1] for n in norm], [n[2] for n in norm]
    ref = [float(np.quantile(y, 0.25)) for y in (y0, y1)]
    b = w.bounds_array()
    eng.generate_candidates(w.M, b[:, 0], b[:, 1], 20240601)
    for j in range(2):
        eng.fit(X, norm[j][0], w.kernel, w.length_scale, w.noise, slot=j)
    rs = np.random.RandomState(11)
    draws = {S: make_draws(w, S // 16 if S >= 16 else 1, min(S, 16), rs) for S in samples}
    observed = pareto_front(np.column_stack([y0, y1]), ref)[:128]
    _n_levels, levels, cell_lo, cell_hi = box_decomposition(observed, ref)
    kw = {"y_mean": y_mean, "y_std": y_std}
    t = {"posterior_passes_ms": [], "ehvi_kernel_ms": []}
    for S in samples:
        for k in ("call_ms", "fronts_ms", "score_ms", "select_ms", "qnehvi_step_ms"):
            t[f"S{S}_{k}"] = []
    picks, sizes = {}, {}
    for r in range(warmup + runs):
        keep = r >= warmup

        def timed(key, fn):
            t0 = time.perf_counter()
            out = fn()
            eng.synchronize()
            if keep:
                t[key].append((time.perf_counter() - t0) * 1e3)
            return out

        timed("posterior_passes_ms", lambda: [eng.posterior(j, y_mean[j], y_std[j], fetch=False) for j in range(2)])
        eng.ehvi_argbest(levels, cell_lo, cell_hi)
        if keep:
            t["ehvi_kernel_ms"].append(eng.debug_ehvi_ms())
        for S in samples:
            out = timed(f"S{S}_call_ms", lambda: eng.pfes_argbest(draws=draws[S], return_fronts=True, **kw))
            ms = eng.debug_pfes_stage_ms()
            eng.qnehvi_greedy(draws[S], 1, ref, base=X, **kw)
            step = eng.debug_qnehvi_stage_ms()[2]
            if keep:
                for k, v in zip(("fronts_ms", "score_ms", "select_ms", "qnehvi_step_ms"), ms + (step,)):
                    t[f"S{S}_{k}"].append(v)
            if picks.setdefault(S, out[0]) != out[0]:
                raise RuntimeError("pfes_argbest's pick depends on the run")
            sizes[S] = np.asarray(out[5])
    res = {k: stats(v) for k, v in t.items()}
    res["ehvi_front_size"] = int(observed.shape[0])
    for S in samples:
        strips = float(sizes[S].sum()) * w.M
        score = res[f"S{S}_score_ms"]["median"]
        res[f"S{S}_summary"] = {"n_samples": int(len(sizes[S])), "mean_front_size": float(sizes[S].mean()), "max_front_size": int(sizes[S].max()),
                                "strip_evals_per_s": strips / (score * 1e-3), "score_over_ehvi_kernel": score / res["ehvi_kernel_ms"]["median"],
                                "score_over_qnehvi_step": score / res[f"S{S}_qnehvi_step_ms"]["median"], "pick": int(picks[S])}
    res["shape"] = {"N": w.N, "d": w.d, "M": w.M, "kernel": W.KERNEL_NAMES[w.kernel], "length_scale": w.length_scale, "noise": w.noise,
                    "features": FEATURES}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="C3")
    ap.add_argument("--samples", default="16,64")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pfes_bench.json"))
    args = ap.parse_args()
    samples = [int(v) for v in args.samples.split(",")]
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs,
                        "clock": "stages: HIP events around the kernels; calls: host perf_counter around call + stream synchronise"}}
    with GpEngine(0, debug=True) as eng:
        info = eng.device_info()
        out["device"] = {"name": info.get("name") or info.get("arch"), "arch": info.get("arch"), "compute_units": info.get("compute_units")}
        out[args.shape] = measure(eng, W.ALL[args.shape], samples, args.warmup, args.runs)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
