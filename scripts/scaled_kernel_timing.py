"""MEASUREMENT SCRIPT — what the scaled kernels (ConstantKernel * k + WhiteKernel) cost on one MI355X.

    python scripts/scaled_kernel_timing.py

The C3-shaped posterior pass (N = 4096, d = 16, M = 2^20) and fit with an unscaled and a scaled slot, and one log-marginal-likelihood
evaluation at N = 4096, unscaled (gpbo_lml) and scaled (gpbo_lml_scaled: value + the n_ls + 2 gradient components; value alone).
Per call the wall clock around the synchronous call and the HIP-event time of its launches (GpEngine.last_timings: "posterior_main" +
"posterior_finalize" for a posterior pass, "fit" for a fit or an evaluation); median / min / max of 5 after 2 warm-ups.  Prints one
JSON object (profiles/scaled_kernel.json)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCALED = {"amplitude": 7.0, "white": 2e-3}


def stats(values):
    return {"median_ms": float(np.median(values)), "min_ms": float(min(values)), "max_ms": float(max(values))}


def measure(eng, call, event_keys, n=5, warm=2):
    """{"wall": ..., "event": ...} of `call`, the event time summed over `event_keys` of last_timings()."""
    for _ in range(warm):
        call()
    wall, event = [], []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        timings = eng.last_timings()
        event.append(sum(float(timings[k]) for k in event_keys))
    return {"wall": stats(wall), "event": stats(event)}


def main():
    from bayesianoptimization_amd import workloads as W
    from bayesianoptimization_amd.engine import GpEngine

    w = W.C3
    X, y, _ = W.make_observations(w)
    Xc = W.make_candidates(w.bounds_array(), w.M, 7)
    ym, ys = float(np.mean(y)), float(np.std(y))
    yn = (y - ym) / ys
    ls = np.full(w.d, w.length_scale)
    out = {}
    with GpEngine(0) as eng:
        eng.set_candidates(Xc)

        def post():
            eng.posterior(0, ym, ys, fetch=False)
            eng.synchronize()

        for name, kw in (("unscaled", {}), ("scaled_c7_w2e-3", SCALED)):
            eng.fit(X, yn, w.kernel, w.length_scale, w.noise, slot=0, **kw)
            out["posterior_C3_" + name] = measure(eng, post, ("posterior_main", "posterior_finalize"))
            out["fit_C3_" + name] = measure(eng, lambda kw=kw: eng.fit(X, yn, w.kernel, w.length_scale, w.noise, slot=0, **kw), ("fit",))
        out["lml_grad_N4096_unscaled"] = measure(eng, lambda: eng.lml(X, yn, w.kernel, ls, w.noise), ("fit",))
        out["lml_grad_N4096_scaled"] = measure(eng, lambda: eng.lml(X, yn, w.kernel, ls, w.noise, scaled=True, **SCALED), ("fit",))
        out["lml_value_N4096_scaled"] = measure(
            eng, lambda: eng.lml(X, yn, w.kernel, ls, w.noise, eval_gradient=False, scaled=True, **SCALED), ("fit",))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
