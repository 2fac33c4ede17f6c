"""gpmo3_nhvi_greedy — greedy batch noisy expected hypervolume improvement for THREE objectives over a resident (3, T, M) block of
posterior draws (include/gpmo3.h) — next to the 3 G plain gpbo_sample_paths calls it stands for, to gpbo_qnhvi_greedy's score kernel
on two of the objectives in the same process, and to the same greedy step in NumPy on fetched values, at N = 4096, d = 16, M = 2^20
(the C3 shape of BASELINE.json), F = 1024 features, q = 8 picks, T = 64 (4 x 16) and T = 256 (16 x 16) draws, the N observed points as
base.

    python scripts/qnehvi3_bench.py [--shape C3] [--warmup 1] [--runs 3] [--q 8] [--numpy-m 16384] [--out FILE.json]

Protocol (as scripts/qnehvi_bench.py): random data (workloads.make_observations; objectives 1 and 2 are other smooth functions of the
same points), candidates from the device generator, the reference point at the objectives' lower quartiles, `warmup` untimed rounds,
then the median of `runs` timed ones with min / max beside it; ONE process on ONE device, all timed calls alternating in one loop.
Per T:
  call_ms / draws_ms / build_ms / steps_ms   the whole qnehvi3_greedy call (host clock) and its stages (HIP events,
                                             gpmo3_debug_stage_ms): the draws, the front and cell build, the q greedy steps;
                                             step_ms = steps_ms / q
  cells_before / cells_after                 mean cells per draw before the first pick and after the last (front points beside them)
  first_step_ms                              a q = 1 call's stage 3 (median of 3): the ONE step whose cells are known exactly, so
                                             first_step_fp64_gops = 11 * cells_before * T * M / first_step_ms (per cell and candidate:
                                             2 min, 3 subtract, 3 clamp, 2 multiply, 1 add), with the step's selection and update
                                             inside the time; m2_first_step_fp64_gops: gpbo_qnhvi_greedy's, 7 per strip, same loop
  step_bytes, step_gbps                      what one step must move, from the shapes (24 T M + 8 M + 8 M + M), over step_ms, and its
                                             share of copy_peak_gbps (gpbo_hbm_copy_peak in this process)
  sample_paths_ms, call_over_sample_paths    the 3 G plain sample_paths calls over the same groups, host clock; the spread of
                                             call_ms and sample_paths_ms is the run-to-run spread of this run
and once, at T = 64 over `numpy-m` candidates: ONE greedy step in NumPy (the cell sum, the t loop, the division, argmin) on the
fetched values and cells, next to the device's step at that M.  The picks of every run must agree, and the NumPy step must pick the
device's first pick.  Prints one JSON object.
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
from bayesianoptimization_amd.thompson import spectral_draw  # noqa: E402

CASES = (("T64", 4, 16), ("T256", 16, 16))
FEATURES = 1024
PATH_NOISE = 1e-2
OPS_PER_CELL, OPS_PER_STRIP = 11, 7


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def numpy_keys(values, cells, counts):
    _, T, M = values.shape
    total = np.zeros(M)
    for t in range(T):
        f0, f1, f2 = values[:, t]
        hvi = np.zeros(M)
        for x_lo, x_hi, y_lo, y_hi, h in cells[t, :counts[t]]:
            w, v, u = np.minimum(f0, x_hi) - x_lo, np.minimum(f1, y_hi) - y_lo, f2 - h
            hvi = hvi + (np.where(w > 0, w, 0.0) * np.where(v > 0, v, 0.0)) * np.where(u > 0, u, 0.0)
        total = total + hvi
    return -(total / float(T))


def measure(eng, w, warmup, runs, q, numpy_m):
    X, y0, _ = W.make_observations(w)
    b = w.bounds_array()
    u = (X - b[:, 0]) / (b[:, 1] - b[:, 0])
    ys = [y0, np.cos(3.0 * X.sum(1) + 0.7) + 0.1 * np.random.RandomState(5).standard_normal(w.N),
          np.sin(3.0 * u[:, 0]) + np.cos(2.0 * u[:, 1:4].sum(1))]
    norm = [W.normalize_targets(y) for y in ys]
    y_mean, y_std = [n[1] for n in norm], [n[2] for n in norm]
    ref = [float(np.quantile(y, 0.25)) for y in ys]
    eng.generate_candidates(w.M, b[:, 0], b[:, 1], 20240601)
    for j in range(3):
        eng.fit(X, norm[j][0], w.kernel, w.length_scale, w.noise, slot=j)
    rs = np.random.RandomState(11)
    draws = {}
    for name, G, S in CASES:
        draws[name] = [[(*spectral_draw(w.kernel, FEATURES, w.d, rs), rs.standard_normal((S, FEATURES)),
                         rs.standard_normal((S, w.N)) * np.sqrt(PATH_NOISE)) for _ in range(G)] for _ in range(3)]
    kw = {"base": X, "y_mean": y_mean, "y_std": y_std}
    kw2 = {"base": X, "y_mean": y_mean[:2], "y_std": y_std[:2]}
    t, picks, last, copy_peak = {}, {}, {}, []
    for r in range(warmup + runs):
        keep = r >= warmup

        def timed(key, fn):
            t0 = time.perf_counter()
            res = fn()
            eng.synchronize()
            if keep:
                t.setdefault(key, []).append((time.perf_counter() - t0) * 1e3)
            return res

        for name, G, S in CASES:
            out = timed(f"{name}_call_ms", lambda: eng.qnehvi3_greedy(draws[name], q, ref, return_fronts=True, **kw))
            if keep:
                for k, v in zip(("draws_ms", "build_ms", "steps_ms"), eng.debug_qnehvi3_stage_ms()):
                    t.setdefault(f"{name}_{k}", []).append(v)
            if picks.setdefault(name, out["index"].tolist()) != out["index"].tolist():
                raise RuntimeError("qnehvi3_greedy's picks depend on the run")
            last[name] = out
            timed(f"{name}_sample_paths_ms",
                  lambda: [eng.sample_paths(*g, slot=j, y_mean=y_mean[j], y_std=y_std[j]) for j in range(3) for g in draws[name][j]])
            one = eng.qnehvi3_greedy(draws[name], 1, ref, return_fronts=True, **kw)
            two = eng.qnehvi_greedy(draws[name][:2], 1, ref[:2], return_fronts=True, **kw2)
            if keep:
                t.setdefault(f"{name}_first_step_ms", []).append(eng.debug_qnehvi3_stage_ms()[2])
                t.setdefault(f"{name}_m2_first_step_ms", []).append(eng.debug_qnehvi_stage_ms()[2])
            if one["index"][0] != out["index"][0] or not np.array_equal(one["cell_count"][0], out["cell_count"][0]):
                raise RuntimeError("the q = 1 call's first pick or cells differ from the q-step call's")
            last[name + "_m2_strips"] = float(np.mean(two["front_size"][0] + 1))
        if keep:
            copy_peak.append(eng.hbm_copy_peak(1 << 30))
    peak = float(np.median(copy_peak))
    res = {"copy_peak_gbps": stats(copy_peak)}
    for name, G, S in CASES:
        T = G * S
        out = last[name]
        med = lambda k: float(np.median(t[f"{name}_{k}"]))
        step_ms, first_ms, call = med("steps_ms") / q, med("first_step_ms"), med("call_ms")
        step_bytes = 24 * T * w.M + 8 * w.M + 8 * w.M + w.M
        cells = [float(np.mean(out["cell_count"][k])) for k in range(2)]
        gops = OPS_PER_CELL * cells[0] * T * w.M / (first_ms * 1e-3) / 1e9
        gops2 = OPS_PER_STRIP * last[name + "_m2_strips"] * T * w.M / (med("m2_first_step_ms") * 1e-3) / 1e9
        res[name] = {"n_groups": G, "n_paths": S, "n_draws": T, "q": q, "n_base": w.N, "block_bytes": 24 * T * w.M,
                     **{k: stats(t[f"{name}_{k}"]) for k in ("call_ms", "draws_ms", "build_ms", "steps_ms", "first_step_ms",
                                                             "m2_first_step_ms", "sample_paths_ms")},
                     "step_ms": step_ms, "step_bytes": step_bytes, "step_gbps": step_bytes / (step_ms * 1e-3) / 1e9,
                     "step_share_of_copy_peak": step_bytes / (step_ms * 1e-3) / 1e9 / peak,
                     "first_step_gbps": step_bytes / (first_ms * 1e-3) / 1e9,
                     "cells_before": cells[0], "cells_after": cells[1], "cells_max": [int(out["cell_count"][k].max()) for k in range(2)],
                     "front_points_before": float(np.mean(out["front_size"][0])), "front_points_after": float(np.mean(out["front_size"][1])),
                     "first_step_fp64_gops": gops, "m2_strips_before": last[name + "_m2_strips"], "m2_first_step_fp64_gops": gops2,
                     "fp64_rate_over_m2": gops / gops2, "steps_share_of_call": med("steps_ms") / call,
                     "call_over_sample_paths": call / med("sample_paths_ms"),
                     "picks": [int(v) for v in out["index"]], "gains": [float(v) for v in out["gain"]]}
    name, G, S = CASES[0]
    eng.generate_candidates(numpy_m, b[:, 0], b[:, 1], 20240601)
    out = eng.qnehvi3_greedy(draws[name], 1, ref, return_values=True, return_fronts=True, **kw)
    dev_step = eng.debug_qnehvi3_stage_ms()[2]
    t0 = time.perf_counter()
    key = numpy_keys(out["values"], out["cells"][0], out["cell_count"][0])
    i = int(np.argmin(key))
    np_ms = (time.perf_counter() - t0) * 1e3
    if i != out["index"][0] or -key[i] != out["gain"][0]:
        raise RuntimeError("the NumPy step's pick differs from the device's first pick")
    res["numpy_step"] = {"n_draws": G * S, "M": numpy_m, "numpy_step_ms": np_ms, "device_step_ms": dev_step,
                         "numpy_step_over_device_step": np_ms / dev_step}
    res["shape"] = {"N": w.N, "d": w.d, "M": w.M, "kernel": W.KERNEL_NAMES[w.kernel], "length_scale": w.length_scale, "noise": w.noise,
                    "n_features": FEATURES, "path_noise": PATH_NOISE, "ref": ref}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="C3")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--q", type=int, default=8)
    ap.add_argument("--numpy-m", type=int, default=1 << 14)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs,
                        "clock": "stages: HIP events on the context's stream; calls and sample_paths: host perf_counter around call + "
                                 "stream synchronise; numpy: host perf_counter, one run of one step"}}
    with GpEngine(0, debug=True) as eng:
        info = eng.device_info()
        out["device"] = {"name": info.get("name") or info.get("arch"), "arch": info.get("arch"), "compute_units": info.get("compute_units")}
        out[args.shape] = measure(eng, W.ALL[args.shape], args.warmup, args.runs, args.q, args.numpy_m)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
