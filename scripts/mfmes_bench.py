"""gpmf_mes_argbest — multi-fidelity max-value entropy search: the paired posterior pass and its arg-best — next to the yardstick it is
held against: TWO fp64-slab posterior passes of the same box.  N = 4096, d = 16 + 1 fidelity column (the C3 shape of BASELINE.json
with one more input), Matern-2.5, M = 2^20, S = 16 / 64 sampled maxima; the pair pass again at N = 512 and 1536.

    python scripts/mfmes_bench.py [--sizes 4096,512,1536] [--samples 16,64] [--dims 4,8,16] [--warmup 1] [--runs 3] [--out profiles/mfmes_bench.json]

Protocol: random data (workloads.make_observations, candidates from the device generator), `warmup` untimed rounds,
then the median of `runs` timed ones with min / max beside it; everything in ONE process on ONE device, all timed calls in alternation
inside one loop.  TWO engines on the same device hold the same fit and candidates.  The RELEASE library gives the host-clock figures:
the whole gpmf_mes_argbest call and one gpbo_posterior pass on its default route, each a clock around a call that ends in a stream
synchronise.  The DEBUG library (the same sources) gives only what the release one cannot: the pair pass and the selection as KERNEL
times from HIP events (gpmf_debug_stage_ms) and, at the first size, a posterior pass forced to the fp64 slab GEMM
(GPBO_POST_KERNEL=3, read by the debug library per pass; host clock).  gpbo_mfma_f64_peak is measured before and after the loop.
`--dims`: the pair pass again at the first size and the first S with d = 4, 8, 16 inputs (width tiers DP = 4, 8, 16; the main shape's
d = 17 is DP = 32).  The MFMA work does not depend on d and the distance part of the k* generation is proportional to DP, so a line
through the four times splits the kernel into a part per DP and the rest ("generation_fit").  Prints one JSON object.
"""
import argparse
import dataclasses
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


def measure(eng, dbg, w, samples, warmup, runs, slab, pair_only=False):
    """eng: the release library's engine (host clocks), dbg: the debug library's (HIP-event stage times, forced slab route)"""
    X, y, _ = W.make_observations(w)
    yn, ym, ys = W.normalize_targets(y)
    b = w.bounds_array()
    for e in (eng, dbg):
        e.generate_candidates(w.M, b[:, 0], b[:, 1], 20240601)
        e.fit(X, yn, w.kernel, w.length_scale, w.noise)
    fid, target = w.d - 1, float(b[w.d - 1, 1])
    y_star = float(np.max(y)) + 0.1 * ys * np.arange(1, 65)
    t = {"posterior_default_ms": []}
    if slab:
        t["posterior_slab_f64_ms"] = []
    for S in samples:
        t[f"S{S}_pair_ms"], t[f"S{S}_select_ms"], t[f"S{S}_call_ms"] = [], [], []
    picks = {}
    for r in range(warmup + runs):
        keep = r >= warmup

        def timed(key, fn, on=eng):
            t0 = time.perf_counter()
            out = fn()
            on.synchronize()
            if keep:
                t[key].append((time.perf_counter() - t0) * 1e3)
            return out

        if not pair_only:
            timed("posterior_default_ms", lambda: eng.posterior(0, ym, ys, fetch=False))
        if slab:
            os.environ["GPBO_POST_KERNEL"] = "3"
            try:
                timed("posterior_slab_f64_ms", lambda: dbg.posterior(0, ym, ys, fetch=False), on=dbg)
            finally:
                del os.environ["GPBO_POST_KERNEL"]
        for S in samples:
            call = lambda e: e.mf_mes_argbest(y_star[:S], fid, target, 1.0, 1.0, y_mean=ym, y_std=ys)[0]  # noqa: E731
            best = call(dbg)
            ms = dbg.debug_mf_stage_ms()
            if keep:
                t[f"S{S}_pair_ms"].append(ms[0])
                t[f"S{S}_select_ms"].append(ms[1])
            if not pair_only and timed(f"S{S}_call_ms", lambda: call(eng)) != best:
                raise RuntimeError("the release and the debug library pick different candidates")
            if picks.setdefault(S, best) != best:
                raise RuntimeError("mf_mes_argbest's pick depends on the run")
    out = {k: stats(v) for k, v in t.items() if v}
    out["picks"] = {str(S): int(v) for S, v in picks.items()}
    out["pair_flops"] = 2.0 * w.N * w.N * w.M            # two members x N^2 / 2 multiply-adds x 2 flops (the triangle)
    out["shape"] = {"N": w.N, "d": w.d, "M": w.M, "kernel": W.KERNEL_NAMES[w.kernel], "length_scale": w.length_scale, "noise": w.noise}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,512,1536")
    ap.add_argument("--samples", default="16,64")
    ap.add_argument("--dims", default="4,8,16", help="further input widths for the pair pass at the first size ('' for none)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mfmes_bench.json"))
    args = ap.parse_args()
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs,
                        "clock": "pair pass, selection: HIP events around the kernels, DEBUG library; default-route posterior pass and "
                                 "whole calls: host perf_counter around call + stream synchronise, RELEASE library; slab-route posterior "
                                 "pass: the same host clock, DEBUG library (the route can only be forced there)"}}
    samples = [int(v) for v in args.samples.split(",")]
    sizes = [int(v) for v in args.sizes.split(",")]
    with GpEngine(0) as eng, GpEngine(0, debug=True) as dbg:
        info = eng.device_info()
        out["device"] = {"name": info.get("name") or info.get("arch"), "arch": info.get("arch"), "compute_units": info.get("compute_units")}
        out["mfma_f64_peak_tflops"] = [eng.mfma_f64_peak()]
        for i, N in enumerate(sizes):
            w = dataclasses.replace(W.ALL["C3"], name=f"C3+fid N={N}", d=17, N=N, bounds=())
            out[f"N{N}"] = measure(eng, dbg, w, samples if i == 0 else samples[:1], args.warmup, args.runs, slab=(i == 0))
        out["mfma_f64_peak_tflops"].append(eng.mfma_f64_peak())
        dims = [int(v) for v in args.dims.split(",") if v]
        if dims:
            key, dp_of = f"S{samples[0]}_pair_ms", lambda d: max(4, 1 << (d - 1).bit_length())      # the width tiers: 4, 8, 16, 32, 64
            dp, ms = [dp_of(17)], [out[f"N{sizes[0]}"][key]["median"]]
            for d in dims:
                w = dataclasses.replace(W.ALL["C3"], name=f"d={d} N={sizes[0]}", d=d, N=sizes[0], bounds=())
                out[f"N{sizes[0]}_d{d}"] = measure(eng, dbg, w, samples[:1], args.warmup, args.runs, slab=False, pair_only=True)
                dp.append(dp_of(d))
                ms.append(out[f"N{sizes[0]}_d{d}"][key]["median"])
            slope, rest = np.polyfit(dp, ms, 1)
            out["generation_fit"] = {"DP": dp, "pair_ms": ms, "ms_per_DP": float(slope), "rest_ms": float(rest),
                                     "distance_share_at_DP32": float(slope * 32 / ms[0]),
                                     "note": "least squares line pair_ms = rest + ms_per_DP * DP over the width tiers; rest holds the MFMAs, "
                                             "the kernel function's two evaluations per point and the score"}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
