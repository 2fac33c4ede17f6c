"""gpnn_acq_argbest — nearest-neighbour GP scoring of the resident candidates — stage by stage at d = 16, M = 2^20, N = 16384 /
65536 / 262144 observations and k = 16 / 32 / 64 neighbours, next to ONE exact posterior pass at N = 4096 over the same candidates
(the C3 shape of BASELINE.json): the yardstick users know.

    python scripts/nngp_bench.py [--sizes 16384,65536,262144] [--neighbors 16,32,64] [--warmup 1] [--runs 3] [--out profiles/nngp_bench.json]

Protocol, as scripts/sur_bench.py: random data, `warmup` untimed rounds, then the median of `runs` timed ones with
min / max beside it; ONE process, ONE device.  The stages (upload and scaling | neighbour search | local solves | selection) are
KERNEL times from HIP events (gpnn_debug_stage_ms; debug library — the same sources as the product).  The search is reported as a
fraction of its own fp64 VALU work: M N 2 DP flop (a subtraction and an fma count as the fma's two; DP = d = 16 here) over the
vector rate compute_units x 128 flop per clock x the shader clock `mfma_f64_probe` measures in the same process.  The exact pass is
the host clock around `posterior(fetch=False)` + `synchronize()`.  Prints one JSON object.
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

STAGES = ("upload_ms", "search_ms", "solve_ms", "select_ms")


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def measure(eng, w, sizes, neighbors, warmup, runs, valu_tflops):
    rng = np.random.RandomState(20240601)
    b = w.bounds_array()
    eng.generate_candidates(w.M, b[:, 0], b[:, 1], 20240601)
    out = {}
    # the yardstick: one exact posterior pass at the shape's own N over the same candidates
    X, y, _ = W.make_observations(w)
    yn, ym, ys = W.normalize_targets(y)
    eng.fit(X, yn, w.kernel, w.length_scale, w.noise)
    exact = []
    for r in range(warmup + runs):
        eng.synchronize()
        t0 = time.perf_counter()
        eng.posterior(0, ym, ys, fetch=False)
        eng.synchronize()
        if r >= warmup:
            exact.append((time.perf_counter() - t0) * 1e3)
    out[f"exact_posterior_N{w.N}_ms"] = stats(exact)
    for N in sizes:
        Xn = b[:, 0] + rng.uniform(size=(N, w.d)) * (b[:, 1] - b[:, 0])
        yv = np.sin(3.0 * Xn.sum(1)) + 0.1 * rng.standard_normal(N)
        yv = (yv - yv.mean()) / yv.std()
        for k in neighbors:
            t = {s: [] for s in STAGES}
            call, picks = [], set()
            for r in range(warmup + runs):
                eng.synchronize()
                t0 = time.perf_counter()
                best = eng.nn_acq_argbest(Xn, yv, w.kernel, w.length_scale, w.noise, k, UCB, 2.576)[0]
                dt = (time.perf_counter() - t0) * 1e3
                picks.add(int(best))
                if r >= warmup:
                    call.append(dt)
                    for s, v in zip(STAGES, eng.debug_nn_stage_ms()):
                        t[s].append(v)
            if len(picks) != 1:
                raise RuntimeError("nn_acq_argbest's pick depends on the run")
            key = f"N{N}_k{k}"
            out[key] = {s: stats(v) for s, v in t.items()}
            out[key]["call_ms"] = stats(call)
            search = out[key]["search_ms"]["median"]
            flop = float(w.M) * N * 2 * w.d
            out[key]["search_tflops"] = flop / (search * 1e-3) / 1e12
            out[key]["search_fraction_of_valu_rate"] = out[key]["search_tflops"] / valu_tflops
            out[key]["solve_ns_per_candidate"] = out[key]["solve_ms"]["median"] * 1e6 / w.M
            out[key]["kernels_over_exact_N4096_pass"] = (search + out[key]["solve_ms"]["median"]) / out[f"exact_posterior_N{w.N}_ms"]["median"]
            out[key]["pick"] = picks.pop()
    out["shape"] = {"d": w.d, "M": w.M, "kernel": W.KERNEL_NAMES[w.kernel], "length_scale": w.length_scale, "noise": w.noise}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="C3")
    ap.add_argument("--sizes", default="16384,65536,262144")
    ap.add_argument("--neighbors", default="16,32,64")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nngp_bench.json"))
    args = ap.parse_args()
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs, "clock": "stages: HIP events around the kernels; calls and the exact pass: host clock",
                        "yardstick": "the search's own fp64 VALU work over compute_units x 128 flop / clock x the measured shader clock; "
                                     "one exact posterior pass at N = 4096 over the same candidates"}}
    with GpEngine(0, debug=True) as eng:
        info = eng.device_info()
        probe = eng.mfma_f64_probe()
        valu_tflops = info["compute_units"] * 128 * probe["shader_mhz"] * 1e6 / 1e12
        out["device"] = {"name": info.get("name") or info.get("arch"), "arch": info.get("arch"), "compute_units": info.get("compute_units"),
                         "shader_mhz": probe["shader_mhz"], "valu_f64_tflops": valu_tflops}
        out[args.shape] = measure(eng, W.ALL[args.shape], [int(v) for v in args.sizes.split(",")],
                                  [int(v) for v in args.neighbors.split(",")], args.warmup, args.runs, valu_tflops)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
