"""gpbo_ascend_paths — 16 posterior function draws, each climbed from its 4 best candidates to a local maximiser in one launch —
next to gpbo_sample_paths on the same inputs and to SciPy L-BFGS-B over a NumPy restatement of the draws (the only way a user
has to refine a draw without it), at the C2 (N = 512, d = 8, M = 65 536) and C3 (N = 4096, d = 16, M = 2^20) shapes of BASELINE.json.

    python scripts/path_ascent_bench.py [--shapes C2,C3] [--features 1024] [--starts 4] [--warmup 3] [--runs 10] [--out FILE.json]

Protocol: random data (workloads.make_observations, candidates from the device generator), `warmup` untimed rounds,
then the median of `runs` timed ones with min / max beside it; every timing is a host clock around a call that ends in a stream
synchronise (uploads and fetches inside); ONE process, ONE device, the timed calls in alternation inside one loop.  Per round:
sample_paths, 16 paths [timed] -> ascend_paths with starts=None: the candidate pass, the 16 x K selection and the 16 x K runs [timed]
-> ascend_paths from the same starts given explicitly: the path weights and the runs alone [timed; the same bits asserted] -> the
same with max_iter = 0: one evaluation per run [timed].  `us_per_evaluation` = (explicit-starts call - the max_iter = 0 call) / (the
longest run's evaluations - 1): what one more evaluation of the longest run costs the call.  Once, outside the loop: SciPy L-BFGS-B
with the analytic gradient over the NumPy restatement from the same 16 x K starts on the host [timed once], its best values next to
the device's.  `gain_y_std` = mean over the draws of (refined value - best candidate's value) / y_std.  Prints one JSON object.
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

S = 16


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def _kernel(kind, r):
    """(k(r), slope(r)): dk / dxs_t = slope * (xs_t - Xs_t) — include/gpbo.h"""
    if kind == 0:
        k = np.exp(-0.5 * r * r)
        return k, -k
    if kind == 1:
        s = np.sqrt(5.0) * r
        e = np.exp(-s)
        return (1.0 + s + s * s / 3.0) * e, -(5.0 / 3.0) * (1.0 + s) * e
    if kind == 2:
        s = np.sqrt(3.0) * r
        e = np.exp(-s)
        return (1.0 + s) * e, -3.0 * e
    e = np.exp(-r)
    with np.errstate(divide="ignore", invalid="ignore"):
        return e, np.where(r > 0, -e / r, 0.0)


class HostPaths:
    """The draws restated in NumPy (include/gpbo.h's formulas): V by a Cholesky solve, value and gradient of path s at one point."""

    def __init__(self, kind, X, yn, ls, noise, omega, phase, weights, eps, y_mean, y_std):
        from scipy.linalg import cho_factor, cho_solve
        from scipy.spatial.distance import cdist

        self.kind, self.ls, self.omega, self.phase, self.w = kind, ls, omega, phase, weights
        self.fs, self.ym, self.ys = np.sqrt(2.0 / omega.shape[0]), y_mean, y_std
        self.Xs = X / ls
        K = _kernel(kind, cdist(self.Xs, self.Xs))[0]
        K[np.diag_indices_from(K)] = 1.0 + noise
        t = self.Xs @ omega.T + phase[None, :]
        U = self.fs * (np.cos(2.0 * np.pi * (t - np.rint(t))) @ weights.T) + eps.T
        self.V = cho_solve(cho_factor(K, lower=True), yn[:, None] - U)

    def value_grad(self, s, x):
        q = x / self.ls
        t = self.omega @ q + self.phase
        a = 2.0 * np.pi * (t - np.rint(t))
        diff = q[None, :] - self.Xs
        k, sl = _kernel(self.kind, np.sqrt((diff * diff).sum(axis=1)))
        f = self.fs * (self.w[s] @ np.cos(a)) + k @ self.V[:, s]
        g = (-2.0 * np.pi * self.fs) * ((self.w[s] * np.sin(a)) @ self.omega) + (sl * self.V[:, s]) @ diff
        return self.ys * f + self.ym, self.ys * g / self.ls


def scipy_runs(host, starts, lo, hi):
    from scipy.optimize import minimize

    S_, K, _ = starts.shape
    f, nfev = np.empty((S_, K)), np.empty((S_, K), dtype=np.int64)
    t0 = time.perf_counter()
    for s in range(S_):
        for k in range(K):
            def neg(x, s=s):
                fv, gv = host.value_grad(s, x)
                return -fv, -gv

            res = minimize(neg, np.clip(starts[s, k], lo, hi), jac=True, bounds=list(zip(lo, hi)), method="L-BFGS-B")
            f[s, k], nfev[s, k] = -res.fun, res.nfev
    return f, nfev, (time.perf_counter() - t0) * 1e3


def measure(eng, w, features, K, warmup, runs):
    X, y, _ = W.make_observations(w)
    yn, ym, ys = W.normalize_targets(y)
    b = w.bounds_array()
    lo, hi = np.ascontiguousarray(b[:, 0]), np.ascontiguousarray(b[:, 1])
    eng.generate_candidates(w.M, lo, hi, 20240601)
    rs = np.random.RandomState(11)
    omega, phase = spectral_draw(w.kernel, features, w.d, rs)
    weights = rs.standard_normal((S, features))
    eps = rs.standard_normal((S, w.N)) * np.sqrt(w.noise)
    ls = np.broadcast_to(np.asarray(w.length_scale, dtype=np.float64), (w.d,))
    eng.fit(X, yn, w.kernel, w.length_scale, w.noise)
    keys = ("sample_paths_ms", "ascend_paths_resident_ms", "ascend_paths_explicit_ms", "ascend_paths_one_evaluation_ms")
    t = {k: [] for k in keys}

    def timed(key, fn, keep):
        t0 = time.perf_counter()
        out = fn()
        eng.synchronize()
        if keep:
            t[key].append((time.perf_counter() - t0) * 1e3)
        return out

    kw = {"y_mean": ym, "y_std": ys}
    first = None
    for r in range(warmup + runs):
        keep = r >= warmup
        timed("sample_paths_ms", lambda: eng.sample_paths(omega, phase, weights, eps, **kw), keep)
        res = timed("ascend_paths_resident_ms", lambda: eng.ascend_paths(omega, phase, weights, eps, lo, hi, n_starts=K, **kw), keep)
        starts = np.asarray(eng.get_candidate_rows(res["start_idx"].ravel(), w.d)).reshape(S, K, w.d)
        exp = timed("ascend_paths_explicit_ms", lambda: eng.ascend_paths(omega, phase, weights, eps, lo, hi, starts=starts, **kw), keep)
        timed("ascend_paths_one_evaluation_ms",
              lambda: eng.ascend_paths(omega, phase, weights, eps, lo, hi, starts=starts, max_iter=0, **kw), keep)
        if not (np.array_equal(res["x"], exp["x"]) and np.array_equal(res["f"], exp["f"])):
            raise RuntimeError("ascend_paths from resident starts and from the same starts given explicitly differ")
        if first is not None and not np.array_equal(first, res["x"]):
            raise RuntimeError("ascend_paths is not repeatable")
        first = res["x"]
    out = {k: stats(v) for k, v in t.items()}
    n_eval = res["n_eval"]
    longest = int(n_eval.max())
    out["evaluations_per_run"] = {"median": float(np.median(n_eval)), "min": int(n_eval.min()), "max": longest, "mean": float(n_eval.mean())}
    out["status_counts"] = np.bincount(res["status"].ravel(), minlength=4).tolist()
    out["us_per_evaluation"] = 1e3 * (out["ascend_paths_explicit_ms"]["median"] - out["ascend_paths_one_evaluation_ms"]["median"]) / max(longest - 1, 1)
    out["us_per_evaluation_whole_call"] = 1e3 * out["ascend_paths_explicit_ms"]["median"] / longest
    out["ascent_over_sample_paths"] = out["ascend_paths_resident_ms"]["median"] / out["sample_paths_ms"]["median"]
    out["gain_y_std"] = float(np.mean((res["f_best"] - res["best_val"]) / ys))
    host = HostPaths(w.kernel, X, yn, ls, w.noise, omega, phase, weights, eps, ym, ys)
    f_host, nfev, ms = scipy_runs(host, starts, lo, hi)
    out["scipy_lbfgsb_host_ms"] = ms
    out["scipy_evaluations_per_run"] = {"median": float(np.median(nfev)), "min": int(nfev.min()), "max": int(nfev.max())}
    out["scipy_over_device"] = ms / out["ascend_paths_explicit_ms"]["median"]
    out["device_best_minus_scipy_best_y_std"] = ((res["f_best"] - f_host.max(axis=1)) / ys).tolist()
    out["shape"] = {"N": w.N, "d": w.d, "M": w.M, "F": features, "paths": S, "starts": K, "kernel": W.KERNEL_NAMES[w.kernel],
                    "length_scale": w.length_scale}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C2,C3")
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--starts", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"protocol": {"warmup": args.warmup, "runs": args.runs, "paths": S, "starts": args.starts, "features": args.features,
                        "clock": "host perf_counter around call + stream synchronise"}}
    with GpEngine(0) as eng:
        out["device"] = eng.device_info().get("name")
        for name in args.shapes.split(","):
            out[name] = measure(eng, W.ALL[name], args.features, args.starts, args.warmup, args.runs)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
