"""gpbo_qnhvi_greedy — greedy batch noisy expected hypervolume improvement for two objectives over a resident (2, T, M) block of
posterior draws — next to the 2 G plain gpbo_sample_paths calls it stands for and to the same greedy step in NumPy on fetched values,
at N = 4096, d = 16, M = 2^20 (the C3 shape of BASELINE.json), F = 1024 features, q = 8 picks, T = 64 (4 x 16) and T = 256 (16 x 16)
draws, the N observed points as base.

    python scripts/qnehvi_bench.py [--shape C3] [--warmup 1] [--runs 5] [--q 8] [--numpy-m 65536] [--out FILE.json]

Protocol: random data (workloads.make_observations; the second objective is cos(3 sum x + 0.7) + 0.1 noise on the same
points), candidates from the device generator, the reference point at the objectives' lower quartiles, `warmup` untimed rounds, then
the median of `runs` timed ones with min / max beside it; everything in ONE process on ONE device, all timed calls in alternation
inside one loop.  Per T:
  call_ms          the whole qnehvi_greedy call, host clock: the upload of the draws' inputs, every kernel, the fetch of the q records
                   and the fronts, the synchronise
  draws_ms         stage 1, HIP events (gpbo_debug_qnehvi_stage_ms, debug library — the same sources as the product): the scalings,
                   per slot and group the path weights and the passes over candidates and base points
  fronts_ms        stage 2, HIP events: qnehvi_front_kernel, T workgroups over the N base pairs
  steps_ms         stage 3, HIP events: the q greedy steps (score + selection + update each); step_ms = steps_ms / q
  step_bytes       what one step must move, from the shapes: both blocks read once (16 T M), the keys written (8 M) and read by the
                   selection (8 M), the mask read (M);  step_gbps = step_bytes / step_ms, and its share of copy_peak_gbps — what
                   gpbo_hbm_copy_peak measures in this process (a copy's read + write bytes per second)
  strips           mean over the draws of (front size + 1), before the first pick and after the last: per pair of loaded values the
                   score kernel walks that many strips, each one 16-byte LDS broadcast and 7 fp64 VALU operations per candidate
  first_step_ms    a q = 1 call's stage 3 (median of 3): the ONE step whose strips are known exactly (strips_before), so
                   first_step_fp64_gops = 7 * strips_before * T * M / first_step_ms is the fp64 operation rate of the score kernel
                   (with the step's selection and update inside the time), and first_step_gbps its bytes over the same time
  sample_paths_ms  baseline (a): the 2 G plain sample_paths calls over the same groups, host clock around them
and once, at T = 64 over `numpy-m` candidates (a size to wait for):
  numpy_step_ms    baseline (b): ONE greedy step (tests/qnehvi_truth.py's arithmetic: per draw the sequential strip loop, the t loop,
                   the division, argmin, the insertions) in NumPy on the fetched values and fronts, ONE run, host clock, next to the
                   device's step at that M
The picks of every run must agree, and the NumPy step must pick the device's first pick.  Prints one JSON object.
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
PATH_NOISE = 1e-2      # the noise the draws' eps are scaled with (normalised-target units)
OPS_PER_STRIP = 7      # min, subtract, clamp, subtract, clamp, multiply, add


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def numpy_step(values, fronts, ref):
    """one greedy step on the host: (pick, gain); the fronts are updated in place"""
    _, T, M = values.shape
    total = np.zeros(M)
    for t in range(T):
        f0, f1, P = values[0, t], values[1, t], fronts[t]
        a = np.concatenate([[np.inf], P[:, 0], [ref[0]]])
        c = np.concatenate([[ref[1]], P[:, 1]])
        hvi = np.zeros(M)
        for k in range(P.shape[0] + 1):
            w = np.minimum(f0, a[k]) - a[k + 1]
            h = f1 - c[k]
            hvi = hvi + np.where(w > 0, w, 0.0) * np.where(h > 0, h, 0.0)
        total = total + hvi
    key = -(total / float(T))
    i = int(np.argmin(key))
    for t in range(T):
        y, P = values[:, t, i], fronts[t]
        if y[0] > ref[0] and y[1] > ref[1] and not np.any((P[:, 0] >= y[0]) & (P[:, 1] >= y[1])):
            keep = P[~((P[:, 0] <= y[0]) & (P[:, 1] <= y[1]))]
            at = int(np.sum(keep[:, 0] > y[0]))
            fronts[t] = np.vstack([keep[:at], y[None], keep[at:]])
    return i, -key[i]


def make_draws(w, G, S, rs):
    draws = []
    for _ in range(2):
        groups = []
        for _ in range(G):
            omega, phase = spectral_draw(w.kernel, FEATURES, w.d, rs)
            groups.append((omega, phase, rs.standard_normal((S, FEATURES)), rs.standard_normal((S, w.N)) * np.sqrt(PATH_NOISE)))
        draws.append(groups)
    return draws


def measure(eng, w, warmup, runs, q, numpy_m):
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
    draws = {name: make_draws(w, G, S, rs) for name, G, S in CASES}
    kw = {"base": X, "y_mean": y_mean, "y_std": y_std}
    t = {f"{name}_{k}": [] for name, _, _ in CASES for k in ("call_ms", "draws_ms", "fronts_ms", "steps_ms", "sample_paths_ms")}
    picks, last = {}, {}
    copy_peak = []
    for r in range(warmup + runs):
        keep = r >= warmup

        def timed(key, fn):
            t0 = time.perf_counter()
            res = fn()
            eng.synchronize()
            if keep:
                t[key].append((time.perf_counter() - t0) * 1e3)
            return res

        for name, G, S in CASES:
            out = timed(f"{name}_call_ms", lambda: eng.qnehvi_greedy(draws[name], q, ref, return_fronts=True, **kw))
            if keep:
                ms = eng.debug_qnehvi_stage_ms()
                for k, v in zip(("draws_ms", "fronts_ms", "steps_ms"), ms):
                    t[f"{name}_{k}"].append(v)
            if picks.setdefault(name, out["index"].tolist()) != out["index"].tolist():
                raise RuntimeError("qnehvi_greedy's picks depend on the run")
            last[name] = out
            timed(f"{name}_sample_paths_ms",
                  lambda: [eng.sample_paths(*g, slot=j, y_mean=y_mean[j], y_std=y_std[j]) for j in range(2) for g in draws[name][j]])
        if keep:
            copy_peak.append(eng.hbm_copy_peak(1 << 30))
    peak = float(np.median(copy_peak))
    res = {"copy_peak_gbps": stats(copy_peak)}
    for name, G, S in CASES:
        T = G * S
        sizes = last[name]["front_size"]
        strips = [float(np.mean(sizes[0] + 1)), float(np.mean(sizes[1] + 1))]
        step_ms = float(np.median(t[f"{name}_steps_ms"])) / q
        step_bytes = 16 * T * w.M + 8 * w.M + 8 * w.M + w.M
        gbps = step_bytes / (step_ms * 1e-3) / 1e9
        call = float(np.median(t[f"{name}_call_ms"]))
        first = []
        for _ in range(3):
            one = eng.qnehvi_greedy(draws[name], 1, ref, return_fronts=True, **kw)
            first.append(eng.debug_qnehvi_stage_ms()[2])
        if one["index"][0] != last[name]["index"][0] or not np.array_equal(one["front_size"][0], sizes[0]):
            raise RuntimeError("the q = 1 call's first pick or fronts differ from the q-step call's")
        first_ms = float(np.median(first))
        res[name] = {"n_groups": G, "n_paths": S, "n_draws": T, "q": q, "n_base": w.N, "block_bytes": 16 * T * w.M,
                     "call_ms": stats(t[f"{name}_call_ms"]), "draws_ms": stats(t[f"{name}_draws_ms"]),
                     "fronts_ms": stats(t[f"{name}_fronts_ms"]), "steps_ms": stats(t[f"{name}_steps_ms"]), "step_ms": step_ms,
                     "step_bytes": step_bytes, "step_gbps": gbps, "step_share_of_copy_peak": gbps / peak,
                     "strips_before": strips[0], "strips_after": strips[1], "front_size_max": [int(sizes[0].max()), int(sizes[1].max())],
                     "first_step_ms": stats(first), "first_step_gbps": step_bytes / (first_ms * 1e-3) / 1e9,
                     "first_step_fp64_gops": OPS_PER_STRIP * strips[0] * T * w.M / (first_ms * 1e-3) / 1e9,
                     "strips_after_first_step": float(np.mean(one["front_size"][1] + 1)),
                     "steps_share_of_call": float(np.median(t[f"{name}_steps_ms"])) / call,
                     "sample_paths_ms": stats(t[f"{name}_sample_paths_ms"]),
                     "call_over_sample_paths": call / float(np.median(t[f"{name}_sample_paths_ms"])),
                     "picks": [int(v) for v in last[name]["index"]], "gains": [float(v) for v in last[name]["gain"]]}
    # the NumPy step, at a size to wait for
    name, G, S = CASES[0]
    eng.generate_candidates(numpy_m, b[:, 0], b[:, 1], 20240601)
    out = eng.qnehvi_greedy(draws[name], 1, ref, return_values=True, return_fronts=True, **kw)
    dev_step = eng.debug_qnehvi_stage_ms()[2]
    fronts = [np.array(out["fronts"][0, t, :int(out["front_size"][0, t])]) for t in range(G * S)]
    t0 = time.perf_counter()
    i, g = numpy_step(out["values"], fronts, ref)
    np_ms = (time.perf_counter() - t0) * 1e3
    if i != out["index"][0] or g != out["gain"][0]:
        raise RuntimeError("the NumPy step's pick differs from the device's first pick")
    if [f.shape[0] for f in fronts] != out["front_size"][1].tolist():
        raise RuntimeError("the NumPy step's fronts differ from the device's")
    res["numpy_step"] = {"n_draws": G * S, "M": numpy_m, "numpy_step_ms": np_ms, "device_step_ms": dev_step,
                         "numpy_step_over_device_step": np_ms / dev_step}
    res["shape"] = {"N": w.N, "d": w.d, "M": w.M, "kernel": W.KERNEL_NAMES[w.kernel], "length_scale": w.length_scale, "noise": w.noise,
                    "n_features": FEATURES, "path_noise": PATH_NOISE, "ref": ref}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="C3")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--q", type=int, default=8)
    ap.add_argument("--numpy-m", type=int, default=1 << 16)
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
