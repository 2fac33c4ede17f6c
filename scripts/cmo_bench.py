"""gpmo_cnhvi_greedy and gpmo_cehvi_argbest (include/gpmo.h) next to the calls they are composed of, at N = 4096, d = 16, M = 2^20
(the C3 shape of BASELINE.json), F = 1024 features, q = 8 picks, T = 64 (4 x 16) and T = 256 (16 x 16) draws, C = 1 and C = 2
constraints, n_base = N observed points.

    python scripts/cmo_bench.py [--shape C3] [--warmup 1] [--runs 3] [--q 8] [--out profiles/cmo_bench.json]

Protocol (as scripts/cnei_bench.py): random data (workloads.make_observations; objective 1 and the constraints' targets are other
smooth functions of the same points), candidates from the device generator, `warmup` untimed rounds, then the median of `runs` timed
ones with min / max beside it; everything in ONE process on ONE device, all timed calls in alternation inside one loop.  Per (T, C):
  call_ms / draws_ms / fronts_ms / steps_ms   the whole cnehvi_greedy call (host clock) and its three stages (HIP events,
                                              gpbo_debug_cnhvi_stage_ms)
  constrained_ms                              the gpbo_sample_paths_constrained calls the draws stand for: per group one call over
                                              (objective 0, the C constraints) and one plain gpbo_sample_paths of objective 1
  draws_over_constrained                      draws_ms / constrained_ms
  steps_over_qnehvi_steps                     steps_ms over gpbo_qnhvi_greedy's at the same T and M (the same front and score kernels)
and per T gpbo_qnhvi_greedy on the same two objectives (qnehvi_call_ms and its stages), re-measured in the same loop.
The value kernels: for a 32-point front at m = 2 and m = 3, ehvi_kernel_ms (gpbo_ehvi_argbest) and cehvi_kernel_ms for C = 1 and 2 in
product and log form (HIP events around the value kernel alone, gpbo_debug_ehvi_ms), with the whole calls' host clocks beside them.
The picks of every run must agree.  Prints one JSON object.
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

LAYOUTS = (("T64", 4, 16), ("T256", 16, 16))
CONSTRAINTS = (1, 2)
FEATURES = 1024
PATH_NOISE = 1e-2      # the noise the draws' eps are scaled with (normalised-target units)
FRONT = 32


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def simplex_front(n, m, lo, hi):
    """n mutually non-dominated points between lo and hi (m,): points of the unit simplex (equal coordinate sums: none dominates)"""
    P = np.random.RandomState(5).dirichlet(np.ones(m), size=n)
    return lo + (hi - lo) * P


def measure(eng, w, warmup, runs, q):
    X, y, _ = W.make_observations(w)
    b = w.bounds_array()
    eng.generate_candidates(w.M, b[:, 0], b[:, 1], 20240601)
    u = (X - b[:, 0]) / (b[:, 1] - b[:, 0])
    targets = [y, np.cos(2.0 * u[:, :3].sum(1)) + u[:, 3], np.sin(3.0 * u[:, 0]) + np.cos(2.0 * u[:, 1:4].sum(1)),
               u[:, 4] * u[:, 5] - np.sin(2.0 * u[:, 6:9].sum(1))]
    n_slots = len(targets)
    y_mean, y_std = np.empty(n_slots), np.empty(n_slots)
    for j, tj in enumerate(targets):
        yn, y_mean[j], y_std[j] = W.normalize_targets(tj)
        eng.fit(X, yn, w.kernel, w.length_scale, w.noise, slot=j)
    lb_all = np.array([-np.inf, y_mean[3] - 0.75 * y_std[3]])
    ub_all = np.array([y_mean[2] + 0.5 * y_std[2], np.inf])
    ref = y_mean[:2] - 2.0 * y_std[:2]
    rs = np.random.RandomState(11)
    draws = {}
    for name, G, S in LAYOUTS:
        draws[name] = [[] for _ in range(n_slots)]
        for j in range(n_slots):
            for _ in range(G):
                omega, phase = spectral_draw(w.kernel, FEATURES, w.d, rs)
                draws[name][j].append((omega, phase, rs.standard_normal((S, FEATURES)), rs.standard_normal((S, w.N)) * np.sqrt(PATH_NOISE)))

    def cnehvi(name, C):
        return eng.cnehvi_greedy(draws[name][:2 + C], q, lb_all[:C], ub_all[:C], ref, base=X, y_mean=y_mean[:2 + C], y_std=y_std[:2 + C])

    def qnehvi(name):
        return eng.qnehvi_greedy(draws[name][:2], q, ref, base=X, y_mean=y_mean[:2], y_std=y_std[:2])

    def constrained(name, C, G):
        # (gpbo_sample_paths_constrained reads the objective in slot 0 and constraint j in slot j; every slot here has the same N, d
        # and kernel, so slot 1's model and inputs stand in for each constraint's pass: the same kernels over the same shapes)
        for g in range(G):
            eng.sample_paths_constrained([draws[name][0][g]] + [draws[name][1][g]] * C, lb_all[:C], ub_all[:C],
                                         y_mean[[0] + [1] * C], y_std[[0] + [1] * C])
            eng.sample_paths(*draws[name][1][g], slot=1, y_mean=y_mean[1], y_std=y_std[1])

    t, picks = {}, {}
    for r in range(warmup + runs):
        keep = r >= warmup

        def timed(key, fn):
            t0 = time.perf_counter()
            res = fn()
            eng.synchronize()
            if keep:
                t.setdefault(key, []).append((time.perf_counter() - t0) * 1e3)
            return res

        def stages(prefix, ms):
            if keep:
                for k, v in zip(("draws_ms", "fronts_ms", "steps_ms"), ms):
                    t.setdefault(prefix + k, []).append(v)

        for name, G, S in LAYOUTS:
            timed(f"{name}_qnehvi_call_ms", lambda: qnehvi(name))
            stages(f"{name}_qnehvi_", eng.debug_qnehvi_stage_ms())
            for C in CONSTRAINTS:
                out = timed(f"{name}_C{C}_call_ms", lambda: cnehvi(name, C))
                stages(f"{name}_C{C}_", eng.debug_cnhvi_stage_ms())
                if picks.setdefault((name, C), out["index"].tolist()) != out["index"].tolist():
                    raise RuntimeError("cnehvi_greedy's picks depend on the run")
                timed(f"{name}_C{C}_constrained_ms", lambda: constrained(name, C, G))
    med = {k: float(np.median(v)) for k, v in t.items()}
    res = {}
    for name, G, S in LAYOUTS:
        T = G * S
        res[name] = {"n_groups": G, "n_paths": S, "n_draws": T, "q": q, "block_bytes": 16 * T * w.M,
                     "qnehvi": {k: stats(t[f"{name}_qnehvi_{k}"]) for k in ("call_ms", "draws_ms", "fronts_ms", "steps_ms")}}
        for C in CONSTRAINTS:
            k = f"{name}_C{C}_"
            out = cnehvi(name, C)
            res[name][f"C{C}"] = {**{s: stats(t[k + s]) for s in ("call_ms", "draws_ms", "fronts_ms", "steps_ms", "constrained_ms")},
                                  "draws_over_constrained": med[k + "draws_ms"] / med[k + "constrained_ms"],
                                  "steps_over_qnehvi_steps": med[k + "steps_ms"] / med[f"{name}_qnehvi_steps_ms"],
                                  "call_over_qnehvi_call": med[k + "call_ms"] / med[f"{name}_qnehvi_call_ms"],
                                  "picks": [int(v) for v in out["index"]], "gains": [float(v) for v in out["gain"]],
                                  "feasible": [float(v) for v in out["feasible"]]}
    # the value kernels: a 32-point front at m = 2 and m = 3; the constraints are slots m .. m + C - 1 (for m = 3: slot 3 alone has a
    # constraint's targets; slot 2 serves as the third objective, and C = 2 is measured at m = 2 only)
    for j in range(n_slots):
        eng.posterior(j, y_mean[j], y_std[j], fetch=False)
    res["ehvi"] = {}
    for m in (2, 3):
        lo = y_mean[:m] - 0.5 * y_std[:m]
        front = pareto_front(simplex_front(FRONT, m, lo, lo + 2.0 * y_std[:m]), y_mean[:m] - 2.0 * y_std[:m])
        _n, levels, c_lo, c_hi = box_decomposition(front, y_mean[:m] - 2.0 * y_std[:m])
        entry = {"front_points": int(front.shape[0]), "n_cells": int(c_lo.shape[0])}
        variants = [("ehvi", None, None)] + [(f"cehvi_C{C}_{'log' if lf else 'product'}", C, lf)
                                             for C in CONSTRAINTS if m + C <= n_slots for lf in (False, True)]
        tk = {v[0]: ([], []) for v in variants}
        for r in range(warmup + runs):
            for key, C, lf in variants:
                t0 = time.perf_counter()
                if C is None:
                    eng.ehvi_argbest(levels, c_lo, c_hi)
                else:
                    sl = slice(0, C) if m == 2 else slice(1, 2)      # the bounds of the constraint models that sit in slots m ..
                    eng.cehvi_argbest(levels, c_lo, c_hi, lb_all[sl], ub_all[sl], log_form=lf)
                eng.synchronize()
                if r >= warmup:
                    tk[key][0].append((time.perf_counter() - t0) * 1e3)
                    tk[key][1].append(eng.debug_ehvi_ms())
        for key, (call, kern) in tk.items():
            entry[key] = {"call_ms": stats(call), "kernel_ms": stats(kern)}
            if key != "ehvi":
                entry[key]["kernel_over_ehvi_kernel"] = float(np.median(kern)) / float(np.median(tk["ehvi"][1]))
        res["ehvi"][f"m{m}"] = entry
    res["shape"] = {"N": w.N, "d": w.d, "M": w.M, "n_base": w.N, "kernel": W.KERNEL_NAMES[w.kernel], "length_scale": w.length_scale,
                    "noise": w.noise, "n_features": FEATURES, "path_noise": PATH_NOISE}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="C3")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--q", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs,
                        "clock": "stages and value kernels: HIP events on the context's stream; calls: host perf_counter around call + "
                                 "stream synchronise"}}
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
