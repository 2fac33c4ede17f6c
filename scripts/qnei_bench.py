"""gpbo_qnei_greedy — greedy batch noisy expected improvement over a resident (T, M) block of posterior draws — next to the G plain
gpbo_sample_paths calls it stands for and to the same greedy step in NumPy on the fetched values, at N = 4096, d = 16, M = 2^20
(the C3 shape of BASELINE.json), F = 1024 features, q = 8 picks, T = 64 (4 x 16) and T = 256 (16 x 16) draws.

    python scripts/qnei_bench.py [--shape C3] [--warmup 1] [--runs 5] [--q 8] [--out FILE.json]

Protocol: random data (workloads.make_observations), candidates from the device generator, `warmup` untimed rounds,
then the median of `runs` timed ones with min / max beside it; everything in ONE process on ONE device, all timed calls in
alternation inside one loop.  Per T:
  call_ms          the whole qnei_greedy call, host clock: the upload of the draws' inputs, every kernel, the fetch of the q records
                   and the T baselines, the synchronise
  draws_ms         stage 1, HIP events (gpbo_debug_qnei_stage_ms, debug library — the same sources as the product): the scaling,
                   per group the path weights and the passes over candidates and training points, the baselines
  steps_ms         stage 2, HIP events: the q greedy steps (score + selection + update each); step_ms = steps_ms / q
  step_bytes       what one step must move, from the shapes: the block read once (8 T M), the keys written (8 M) and read by the
                   selection (8 M), the mask read (M);  step_gbps = step_bytes / step_ms, and its share of copy_peak_gbps — what
                   gpbo_hbm_copy_peak measures in this process (a copy's read + write bytes per second).  The step is bound by
                   memory: per loaded value it does one subtract, one compare / select and one add
  sample_paths_ms  baseline (a): the G plain sample_paths calls over the same groups (each with its own selection of S maximisers),
                   host clock around the G calls
  numpy_step_ms    baseline (b): ONE greedy step (tests/qnei_truth.py's arithmetic: the sequential t loop, the division, the mask,
                   argmin, the fmax update) in NumPy on the fetched (T, M) values, ONE run, host clock; the fetch itself is
                   fetch_values_ms
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


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def numpy_step(values, m):
    """one greedy step on the host: (pick, gain, updated m)"""
    T, M = values.shape
    total = np.zeros(M)
    for t in range(T):
        d = values[t] - m[t]
        total = total + np.where(d > 0, d, np.where(np.isnan(values[t]), values[t], 0.0))
    key = -(total / float(T))
    i = int(np.argmin(key))
    return i, -key[i], np.fmax(m, values[:, i])


def measure(eng, w, warmup, runs, q):
    X, y, _ = W.make_observations(w)
    yn, y_mean, y_std = W.normalize_targets(y)
    b = w.bounds_array()
    eng.generate_candidates(w.M, b[:, 0], b[:, 1], 20240601)
    eng.fit(X, yn, w.kernel, w.length_scale, w.noise)
    rs = np.random.RandomState(11)
    groups = {}
    for name, G, S in CASES:
        groups[name] = []
        for _ in range(G):
            omega, phase = spectral_draw(w.kernel, FEATURES, w.d, rs)
            groups[name].append((omega, phase, rs.standard_normal((S, FEATURES)), rs.standard_normal((S, w.N)) * np.sqrt(PATH_NOISE)))
    t = {f"{name}_{k}": [] for name, _, _ in CASES for k in ("call_ms", "draws_ms", "steps_ms", "sample_paths_ms")}
    picks = {}
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
            out = timed(f"{name}_call_ms", lambda: eng.qnei_greedy(groups[name], q, y_mean=y_mean, y_std=y_std))
            if keep:
                draws, steps = eng.debug_qnei_stage_ms()
                t[f"{name}_draws_ms"].append(draws)
                t[f"{name}_steps_ms"].append(steps)
            if picks.setdefault(name, out[0].tolist()) != out[0].tolist():
                raise RuntimeError("qnei_greedy's picks depend on the run")
            timed(f"{name}_sample_paths_ms",
                  lambda: [eng.sample_paths(*g, y_mean=y_mean, y_std=y_std) for g in groups[name]])
        if keep:
            copy_peak.append(eng.hbm_copy_peak(1 << 30))
    peak = float(np.median(copy_peak))
    out = {"copy_peak_gbps": stats(copy_peak)}
    for name, G, S in CASES:
        T = G * S
        t0 = time.perf_counter()
        idx, gain, m0, values, _ = eng.qnei_greedy(groups[name], q, y_mean=y_mean, y_std=y_std, return_values=True)
        fetch_ms = (time.perf_counter() - t0) * 1e3 - float(np.median(t[f"{name}_call_ms"]))
        t0 = time.perf_counter()
        i, g, _ = numpy_step(values, m0)
        np_ms = (time.perf_counter() - t0) * 1e3
        if i != idx[0] or g != gain[0]:
            raise RuntimeError("the NumPy step's pick differs from the device's first pick")
        del values
        step_ms = float(np.median(t[f"{name}_steps_ms"])) / q
        step_bytes = 8 * T * w.M + 8 * w.M + 8 * w.M + w.M
        gbps = step_bytes / (step_ms * 1e-3) / 1e9
        call = float(np.median(t[f"{name}_call_ms"]))
        out[name] = {"n_groups": G, "n_paths": S, "n_draws": T, "q": q, "block_bytes": 8 * T * w.M,
                     "call_ms": stats(t[f"{name}_call_ms"]), "draws_ms": stats(t[f"{name}_draws_ms"]),
                     "steps_ms": stats(t[f"{name}_steps_ms"]), "step_ms": step_ms, "step_bytes": step_bytes, "step_gbps": gbps,
                     "step_share_of_copy_peak": gbps / peak, "steps_share_of_call": float(np.median(t[f"{name}_steps_ms"])) / call,
                     "sample_paths_ms": stats(t[f"{name}_sample_paths_ms"]),
                     "call_over_sample_paths": call / float(np.median(t[f"{name}_sample_paths_ms"])),
                     "fetch_values_ms": fetch_ms, "numpy_step_ms": np_ms, "numpy_step_over_device_step": np_ms / step_ms,
                     "picks": [int(v) for v in idx], "gains": [float(v) for v in gain]}
    out["shape"] = {"N": w.N, "d": w.d, "M": w.M, "kernel": W.KERNEL_NAMES[w.kernel], "length_scale": w.length_scale, "noise": w.noise,
                    "n_features": FEATURES, "path_noise": PATH_NOISE}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="C3")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--q", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs,
                        "clock": "stages: HIP events on the context's stream; calls and sample_paths: host perf_counter around call + "
                                 "stream synchronise; numpy: host perf_counter, one run of one step"}}
    with GpEngine(0, debug=True) as eng:
        info = eng.device_info()
        out["device"] = {"name": info.get("name") or info.get("arch"), "arch": info.get("arch"), "compute_units": info.get("compute_units")}
        out[args.shape] = measure(eng, W.ALL[args.shape], args.warmup, args.runs, args.q)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
