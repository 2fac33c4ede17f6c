"""gpbo_ehvi_argbest — expected hypervolume improvement over the resident candidates and its arg-best — next to the m posterior passes
that feed it and to the same sum evaluated in NumPy on the fetched mu / sd, at N = 4096, d = 16, M = 2^20 (the C3 shape of
BASELINE.json): m = 2 with a 32-point front, m = 3 with 32- and 128-point fronts.

    python scripts/ehvi_bench.py [--shape C3] [--warmup 2] [--runs 7] [--out FILE.json]

Protocol: random data (workloads.make_observations; objective j's targets are the workload's own, shifted along the
inputs for j > 0), candidates from the device generator, `warmup` untimed rounds, then the median of `runs` timed ones with min / max
beside it; everything in ONE process on ONE device, all timed calls in alternation inside one loop.  Per case:
  kernel_ms      the value kernel alone (tables + sum over the boxes): HIP events around the launch (gpbo_debug_ehvi_ms, debug
                 library — the same sources as the product)
  call_ms        the whole ehvi_argbest call, host clock: the upload of levels and boxes, the kernel, the selection, the synchronise
  posteriors_ms  baseline (a): the m posterior passes that leave the mu / sd the call reads, host clock around the m calls
  numpy_ms       baseline (b): the same tables and the same sum in NumPy / SciPy on the fetched mu / sd, ONE run over the first
                 `numpy_candidates` candidates (the (K, M) temporaries of the whole set do not fit a sensible run), and
                 numpy_ms_scaled_to_M = numpy_ms * M / numpy_candidates beside it — an extrapolation, labelled as such
Fronts: n points on the unit circle / sphere octant, mapped objective by objective between the 35 % and the 97 % quantile of the
fetched posterior means, the reference point a quarter of the means' range below their minimum — the construction of
tests/test_gpu_ehvi.py.  Prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
from scipy import special

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bayesianoptimization_amd import workloads as W  # noqa: E402
from bayesianoptimization_amd.engine import GpEngine  # noqa: E402
from bayesianoptimization_amd.multiobjective import box_decomposition  # noqa: E402

CASES = (("m2_front32", 2, 32, 1 << 16), ("m3_front32", 3, 32, 1 << 16), ("m3_front128", 3, 128, 1 << 12))


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def unit_front(n, m, seed):
    rs = np.random.RandomState(seed)
    if m == 2:
        ang = np.sort(rs.uniform(0.05, 0.5 * np.pi - 0.05, n))
        return np.column_stack([np.cos(ang), np.sin(ang)])
    u = np.abs(rs.standard_normal((n, m))) + 0.05
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def place_front(mu, n, seed):
    m = mu.shape[0]
    lo, hi = np.quantile(mu, 0.35, axis=1), np.quantile(mu, 0.97, axis=1)
    return lo + (hi - lo) * unit_front(n, m, seed), mu.min(axis=1) - 0.25 * np.ptp(mu, axis=1)


def f_numpy(z):
    """f(z) = phi(z) + z Phi(z) over the two ranges of include/gpbo.h"""
    out = np.empty_like(z)
    with np.errstate(all="ignore"):
        up = z > -1.0
        out[up] = np.exp(-(z[up] * z[up]) / 2.0) / 2.50662827463100050242 + z[up] * special.ndtr(z[up])
        zl = z[~up]
        phi = np.exp(-(zl * zl) / 2.0) / 2.50662827463100050242
        near = zl > -28.0
        r = np.empty_like(zl)
        t = -zl[near] * 0.70710678118654752440
        r[near] = 1.0 - 1.77245385090551602730 * t * special.erfcx(t)
        w = 1.0 / (zl[~near] * zl[~near])
        s = np.full_like(w, -654729075.0)
        for c in (34459425.0, -2027025.0, 135135.0, -10395.0, 945.0, -105.0, 15.0, -3.0, 1.0):
            s = s * w + c
        r[~near] = w * s
        out[~up] = np.where(phi == 0.0, 0.0, phi * r)
    return out


def ehvi_numpy(mu, sd, rows, lo, hi):
    value = None
    for j, row in enumerate(rows):
        table = np.stack([np.zeros(mu.shape[1]) if np.isposinf(a) else sd[j] * f_numpy((mu[j] - a) / sd[j]) for a in row])
        factor = table[lo[:, j]] - table[hi[:, j]]
        value = factor if value is None else value * factor
    return value.sum(axis=0)


def measure(eng, w, warmup, runs):
    X, y, _ = W.make_observations(w)
    s = X.sum(axis=1)
    targets = [y, np.roll(y, 1) + 0.3 * np.cos(s), -np.roll(y, 2) + 0.2 * X[:, 0]]
    norm = [W.normalize_targets(t) for t in targets]
    b = w.bounds_array()
    eng.generate_candidates(w.M, b[:, 0], b[:, 1], 20240601)
    for j, (yn, _, _) in enumerate(norm):
        eng.fit(X, yn, w.kernel, w.length_scale, w.noise, slot=j)
    post = [eng.posterior(j, norm[j][1], norm[j][2]) for j in range(3)]
    mu, sd = np.stack([p[0] for p in post]), np.stack([p[1] for p in post])
    boxes, t, out = {}, {}, {}
    for name, m, n, n_np in CASES:
        front, ref = place_front(mu[:m], n, seed=n)
        boxes[name] = box_decomposition(front, ref)
        for k in ("kernel_ms", "call_ms"):
            t[f"{name}_{k}"] = []
    t["posteriors_m2_ms"], t["posteriors_m3_ms"] = [], []
    picks = {}
    for r in range(warmup + runs):
        keep = r >= warmup

        def timed(key, fn):
            t0 = time.perf_counter()
            res = fn()
            eng.synchronize()
            if keep:
                t[key].append((time.perf_counter() - t0) * 1e3)
            return res

        timed("posteriors_m3_ms", lambda: [eng.posterior(j, norm[j][1], norm[j][2], fetch=False) for j in range(3)])
        timed("posteriors_m2_ms", lambda: [eng.posterior(j, norm[j][1], norm[j][2], fetch=False) for j in range(2)])
        for name, m, n, n_np in CASES:
            _, levels, lo, hi = boxes[name]
            best = timed(f"{name}_call_ms", lambda: eng.ehvi_argbest(levels, lo, hi))[0]
            if keep:
                t[f"{name}_kernel_ms"].append(eng.debug_ehvi_ms())
            if picks.setdefault(name, best) != best:
                raise RuntimeError("ehvi_argbest's pick depends on the run")
    for name, m, n, n_np in CASES:
        n_levels, levels, lo, hi = boxes[name]
        rows = [levels[j, :n_levels[j]] for j in range(m)]
        ys = eng.ehvi_argbest(levels, lo, hi, return_values=True)[4]
        t0 = time.perf_counter()
        v = ehvi_numpy(mu[:m, :n_np], sd[:m, :n_np], rows, lo, hi)
        np_ms = (time.perf_counter() - t0) * 1e3
        scale = np.maximum(np.abs(v), 1e-290)
        post_ms = float(np.median(t[f"posteriors_m{m}_ms"]))
        kernel_ms = float(np.median(t[f"{name}_kernel_ms"]))
        out[name] = {"n_objectives": m, "front_size": n, "n_cells": int(lo.shape[0]), "n_levels": [int(v_) for v_ in n_levels],
                     "kernel_ms": stats(t[f"{name}_kernel_ms"]), "call_ms": stats(t[f"{name}_call_ms"]),
                     "posteriors_ms": stats(t[f"posteriors_m{m}_ms"]),
                     "kernel_share_of_posteriors": kernel_ms / post_ms,
                     "call_share_of_posteriors": float(np.median(t[f"{name}_call_ms"])) / post_ms,
                     "numpy_candidates": n_np, "numpy_ms": np_ms, "numpy_ms_scaled_to_M": np_ms * w.M / n_np,
                     "worst_relative_difference_to_numpy": float(np.max(np.abs(-ys[:n_np] - v) / scale)),
                     "pick": int(picks[name])}
    out["shape"] = {"N": w.N, "d": w.d, "M": w.M, "kernel": W.KERNEL_NAMES[w.kernel], "length_scale": w.length_scale, "noise": w.noise}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="C3")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs,
                        "clock": "kernel: HIP events around the launch; calls and posterior passes: host perf_counter around call + "
                                 "stream synchronise; numpy: host perf_counter, one run over numpy_candidates candidates"}}
    with GpEngine(0, debug=True) as eng:
        info = eng.device_info()
        out["device"] = {"name": info.get("name") or info.get("arch"), "arch": info.get("arch"), "compute_units": info.get("compute_units")}
        out[args.shape] = measure(eng, W.ALL[args.shape], args.warmup, args.runs)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
