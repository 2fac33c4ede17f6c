#!/usr/bin/env python
"""bench.py — suggest-step throughput of the HIP GP-posterior + acquisition engine on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config C3] [--dump-outputs DIR]
                    [--full [--no-cpu-baseline] [--no-suggest] [--no-extra-configs]]

A "step" is one pass of the hot path over one batch of synthetic input (BASELINE.json metric,
configs[2] = C3 when it fits one GPU): fit the GP at fixed theta (K, Cholesky, W = L^-1, alpha), then
posterior mu/sigma + acquisition + arg-best/top-10 over M = 2^20 candidates that are already
resident in HBM.  N > 1: every GPU fits redundantly and evaluates its own 2^20-candidate shard (weak
scaling; BASELINE's sharded config C4); the only exchange is an all-gather of 11 (value, index) records
per GPU over RCCL.  Two ways to own the GPUs, same kernels, same exchange:

  * launched by `python -m torch.distributed.run --nproc-per-node N ...` (WORLD_SIZE = N in the environment): one
    process per GPU, ncclCommInitRank; the 128-byte communicator id travels through a file (rendezvous.py), the
    barrier and the max-over-ranks of the wall time are RCCL all-reduces;
  * launched as plain `python bench.py --gpus N`: ONE process, one context + one host thread per GPU
    (gpbo_group_*, ncclCommInitAll) — the shape that sits behind BayesianOptimization.suggest().

No torch anywhere: the product path is ctypes -> libgpbo.so (HIP).  If RCCL cannot be brought up the line says
`"collective": "FAILED"` and the exit status is non-zero — there is no fallback transport.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line: its roofline and step breakdown
are the HIP events of the timed steps themselves.  Everything that takes work of its own goes behind --full: the measured
matrix peak (MFMA probes) and the PMC traffic from profiles/, the stage timings of one fit alone when the fits overlap, parity
with the reference's goldens, the CPU baseline, the other BASELINE.json configs and the ms/suggest measurements.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from bayesianoptimization_amd import rendezvous  # noqa: E402
from bayesianoptimization_amd import workloads as W  # noqa: E402
from bayesianoptimization_amd.distributed import ShardedAcquisition  # noqa: E402
from bayesianoptimization_amd.engine import GpEngine, GroupEngine  # noqa: E402

FP64_MFMA_PEAK_TFLOPS = 78.6  # AMD MI355X datasheet (matrix FP64); the guide lists no fp64 row
FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_*_f32 (f32 in / f32 accumulate)
HBM_ACHIEVABLE_TBPS = 6.29     # MI355X_MICROARCH.md: float4 copy (8.0 spec)
SHARDED = ("C4", "C5")         # quoted as 8-GPU jobs: one eighth of M per GPU
METRIC = "acquisition candidates/sec (suggest step: GP fit at fixed theta + posterior + acquisition + arg-best)"


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def flops_per_candidate(N, d, n_gp=1):
    """F_cand = N^2 + (3d + 12) N per GP (one triangular solve + k* build + mu/sigma)."""
    return n_gp * (float(N) * N + (3.0 * d + 12.0) * N)


def cpu_baseline(w, X, y, c, Xc, y_max, gpu_ys, n_chunks=3):
    """The reference's CPU arithmetic on this box's host cores, on a bounded sample of the same workload.

    kind "reference": /root/reference is mounted (build container) -> the real bayes_opt objects (`_fit_gp`, `_get_acq`
    closure, acquisition.py:79-86, 198-217).  kind "port": the GPU box has no /root/reference -> scikit-learn's
    GaussianProcessRegressor (what bayes_opt delegates to: acquisition.py:84,205,216; constraint.py:148-151,200-221) at the
    same fixed theta + the restated closure from oracle/gp_oracle.py.  Parity is asserted on the very chunks that are timed."""
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, Matern

    from oracle import gp_oracle as O
    from oracle.refenv import have_reference

    chunk = min(8192 if w.N <= 4096 else 2048, Xc.shape[0])
    n_chunks = max(1, min(n_chunks, Xc.shape[0] // chunk))
    kind = "port"
    acq = None
    if have_reference():
        try:
            from oracle.gen_golden import build_reference_objects
            t0 = time.perf_counter()
            opt, fn, _ = build_reference_objects(w)
            fit_s = time.perf_counter() - t0
            acq = fn._get_acq(gp=opt._gp, constraint=opt._space.constraint)
            kind = "reference"
        except Exception as e:  # noqa: BLE001
            log(f"[bench] reference objects unavailable ({e!r}); timing the port")
    if acq is None:
        def mk(ls):
            return RBF(length_scale=ls) if w.kernel == W.RBF else Matern(nu=2.5, length_scale=ls)
        t0 = time.perf_counter()
        gp = GaussianProcessRegressor(kernel=mk(w.length_scale), alpha=w.noise, normalize_y=True, optimizer=None).fit(X, y)
        cgp = None
        if w.constrained:
            cgp = GaussianProcessRegressor(kernel=Matern(nu=2.5, length_scale=w.constraint_length_scale), alpha=w.noise,
                                           normalize_y=True, optimizer=None).fit(X, c)
        fit_s = time.perf_counter() - t0

        def acq(xs):
            mean, std = gp.predict(xs, return_std=True)
            ys = -1 * O.base_acq(w.acq, mean, std, w.acq_param, y_max if y_max is not None else 0.0)
            if cgp is not None:
                cm, cs = cgp.predict(xs, return_std=True)
                ys = ys * O.norm_cdf((w.constraint_ub - cm) / cs)      # lb = -inf -> 0 (constraint.py:202-207)
            return ys
    times, worst = [], 0.0
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for ci in range(n_chunks):
            xs = Xc[ci * chunk:(ci + 1) * chunk]
            t0 = time.perf_counter()
            ys = acq(xs)
            dt = time.perf_counter() - t0
            # a chunk that takes milliseconds (C1: 1024 candidates on 25 observations) is timed again until 0.2 s have gone by
            # and quoted by its median: one 0.3 ms sample is noise, not a baseline (the first call also pays scikit-learn's
            # lazily built predict state)
            reps = [dt]
            while sum(reps) < 0.2 and len(reps) < 200:
                t0 = time.perf_counter()
                acq(xs)
                reps.append(time.perf_counter() - t0)
            times.append(float(np.median(reps)))
            g = gpu_ys[ci * chunk:(ci + 1) * chunk]
            worst = max(worst, float(np.max(np.abs(g - ys)) / np.max(np.abs(ys))))
    if fit_s < 0.05 and kind == "port":      # the same for a fit that takes milliseconds
        fts = []
        while sum(fts) < 0.2 and len(fts) < 50:
            t0 = time.perf_counter()
            GaussianProcessRegressor(kernel=mk(w.length_scale), alpha=w.noise, normalize_y=True, optimizer=None).fit(X, y)
            fts.append(time.perf_counter() - t0)
        fit_s = float(np.median(fts)) * (2 if w.constrained else 1)
    med = float(np.median(times))
    try:
        from threadpoolctl import threadpool_info
        blas_threads = max([p.get("num_threads", 1) for p in threadpool_info()] or [1])
    except Exception:
        blas_threads = os.cpu_count()
    M = Xc.shape[0]
    step_s = fit_s + med * (M / chunk)  # cost is linear in M: extrapolated to the full step
    what = ("bayes_opt 3.3.0 _fit_gp + _get_acq closure" if kind == "reference"
            else f"sklearn {__import__('sklearn').__version__} GaussianProcessRegressor.fit (fixed theta) + "
                 "predict(return_std) + restated acquisition closure")
    return {
        "value": M / step_s, "unit": "candidates/s", "cores": int(blas_threads), "kind": kind,
        "sample": (f"{what}: fit {fit_s:.2f}s + {n_chunks} chunks of {chunk} candidates (median {med:.2f}s/chunk), "
                   f"extrapolated linearly to M={M}; host cpu_count={os.cpu_count()}, BLAS threads={blas_threads}"),
        "acq_pass_value": chunk / med, "fit_s": fit_s,
        "parity_max_rel_vs_gpu_on_timed_chunks": worst,
    }


def suggest_latency(w, X, y, eng, M, reps=3):
    """Median wall time of AcquisitionFunction.suggest(gp, space, n_random=M, n_smart=0|10, fit_gp=True) through
    FloatSpace + HipGPR + the fused acquisition classes (the seams bayes_opt itself calls), the engine
    as the seams' own shared engine runs: no HIP event records (gpbo_set_timing 0)."""
    timing0 = getattr(eng, "timing", True)
    eng.set_timing(False)
    try:
        return _suggest_latency(w, X, y, eng, M, reps)
    finally:
        eng.set_timing(timing0)


def _suggest_latency(w, X, y, eng, M, reps):
    import warnings

    from sklearn.gaussian_process.kernels import Matern, RBF

    from bayesianoptimization_amd import fused_acquisition as A
    from bayesianoptimization_amd.float_space import FloatSpace
    from bayesianoptimization_amd.gpr import HipGPR

    sp = FloatSpace(w.pbounds())
    sp.register_bulk(X, y)
    kern = Matern(nu=2.5, length_scale=w.length_scale) if w.kernel == W.MATERN25 else RBF(length_scale=w.length_scale)
    gp = HipGPR(kernel=kern, alpha=w.noise, normalize_y=True, optimizer=None, engine=eng, incremental=False)  # every call refits
    fn = {W.UCB: lambda: A.UpperConfidenceBound(kappa=w.acq_param), W.EI: lambda: A.ExpectedImprovement(xi=w.acq_param),
          W.POI: lambda: A.ProbabilityOfImprovement(xi=w.acq_param)}[w.acq]()
    res = {}
    fn.device_polish = False          # "n_smart_10" = the reference-shaped local searches (SciPy's iterates, bit parity)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for n_smart in (0, 10):
            ts = []
            for rep in range(reps + 1):
                t0 = time.perf_counter()
                fn.suggest(gp, sp, n_random=M, n_smart=n_smart, fit_gp=True, random_state=np.random.RandomState(7 + rep))
                ts.append((time.perf_counter() - t0) * 1e3)
            res[f"n_smart_{n_smart}"] = float(np.median(ts[1:]))      # first call: allocations
    # the local-search stage as one library call (gpbo_polish_seeds, accelerate(local_search="device")): statistical parity
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fn.device_polish = True
            ts = []
            for rep in range(reps + 1):
                t0 = time.perf_counter()
                fn.suggest(gp, sp, n_random=M, n_smart=10, fit_gp=True, random_state=np.random.RandomState(7 + rep))
                ts.append((time.perf_counter() - t0) * 1e3)
            res["n_smart_10_device_local_search"] = float(np.median(ts[1:]))
    except Exception as e:  # noqa: BLE001
        res["n_smart_10_device_local_search"] = None
        res["device_local_search_error"] = repr(e)
    finally:
        fn.device_polish = False
    res["note"] = ("median of 3 after one warm-up; fixed theta unless the key says otherwise; candidates = the reference's RandomState "
                   "stream, generated on the device; n_smart_10 = SciPy's L-BFGS-B iterates (local_search='reference'), "
                   "n_smart_10_device_local_search = gpbo_polish_seeds (the default of accelerate() since round 4)")
    # ... and as BayesianOptimization itself configures its GP (bayesian_optimization.py: Matern(nu=2.5), alpha=1e-6,
    # normalize_y=True, n_restarts_optimizer=5): every suggest() then also runs sklearn's theta search — 1 + 5 L-BFGS-B
    # runs over the log-marginal likelihood, here with the LML and its gradient on the device (gpbo_lml_batch lanes)
    SEEDS = (100, 101, 102, 103, 104)

    def theta_block(space, tag):
        """default_call & co. over the observations registered in `space`."""
        out = {}
        gp_t = HipGPR(kernel=Matern(nu=2.5), alpha=1e-6, normalize_y=True, n_restarts_optimizer=5,
                      random_state=np.random.RandomState(1), engine=eng, incremental=False)
        stage = {"fit": [], "polish": [], "rounds": [], "evals": []}
        fit0 = gp_t.fit

        def timed_fit(X_, y_):
            t0 = time.perf_counter()
            r = fit0(X_, y_)
            stage["fit"].append((time.perf_counter() - t0) * 1e3)
            stage["rounds"].append(int(getattr(gp_t, "theta_search_rounds_", 0)))
            stage["evals"].append(int(getattr(gp_t, "theta_search_evals_", 0)))
            return r

        gp_t.fit = timed_fit
        polish0 = eng.polish_seeds

        def timed_polish(*a, **k):
            t0 = time.perf_counter()
            r = polish0(*a, **k)
            stage["polish"].append((time.perf_counter() - t0) * 1e3)
            return r

        eng.polish_seeds = timed_polish

        def timed_calls():
            """One warm-up call, then one suggest() per restart seed: call r draws its theta-search restarts from
            RandomState(SEEDS[r]) in EVERY mode (how long a search runs depends on where its restarts start — on the noisy
            generator scikit-learn itself ends 3 of these 5 searches at the lower bound 1e-5 after a few evaluations and 2 at
            the interior optimum after ~20), candidates from RandomState(7 + r)."""
            ts, found = [], []
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for r, seed in enumerate((SEEDS[0],) + SEEDS):
                    gp_t.random_state = np.random.RandomState(seed)
                    t0 = time.perf_counter()
                    fn.suggest(gp_t, space, n_random=M, n_smart=10, fit_gp=True, random_state=np.random.RandomState(7 + r))
                    ts.append((time.perf_counter() - t0) * 1e3)
                    found.append(float(np.exp(gp_t.kernel_.theta[0])))
            return ts[1:], found[1:]

        try:
            if tag == "":
                fn.device_polish = False
                out["n_smart_10_with_theta_search"] = float(np.median(timed_calls()[0]))
            # THE CALL THE REFERENCE MAKES, as accelerate(optimizer) configures it by default: BayesianOptimization's GP (theta
            # search with 5 restarts in every fit, bayesian_optimization.py:124-130; sklearn _gpr.py:296-338) + 10 local
            # searches (acquisition.py:116-169, 322-420), both on the device path
            fn.device_polish = "auto"
            for v in stage.values():
                v.clear()
            ts, found = timed_calls()
            out["default_call"] = float(np.median(ts))
            out["default_call_minus_n_smart_0"] = out["default_call"] - res["n_smart_0"]
            rows = [{"seed": sd, "ms": t, "fit_with_theta_search_ms": f, "theta_search_rounds": rd, "lml_evaluations": ev,
                     "local_search_ms": (stage["polish"][1 + i] if len(stage["polish"]) > 1 + i else None), "length_scale_found": ls}
                    for i, (sd, t, f, rd, ev, ls) in enumerate(zip(SEEDS, ts, stage["fit"][1:], stage["rounds"][1:], stage["evals"][1:], found))]
            out["default_call_per_restart_seed"] = rows
            out["default_call_max"] = float(np.max(ts))
            # the calls whose search did real work: >= 10 lockstep rounds (a search that slides to the lower bound 1e-5 of the length
            # scale in a few evaluations leaves K = I behind, on which the local searches "converge" at once)
            interior = [r_["ms"] for r_ in rows if r_["theta_search_rounds"] >= 10]
            out["default_call_interior"] = float(np.median(interior)) if interior else None
            out["default_call_interior_n"] = len(interior)
            out["default_call_interior_minus_n_smart_0"] = (out["default_call_interior"] - res["n_smart_0"]) if interior else None
        finally:
            del eng.polish_seeds
            fn.device_polish = False
        return out

    try:
        res.update(theta_block(sp, ""))
        if getattr(eng, "last_lane_devices", None) is not None:
            # device group: the theta search's lanes of a lockstep round run on different devices (gpbo_group_lml_batch)
            res["theta_search_lane_devices_last_round"] = list(eng.last_lane_devices)
            distinct = len(set(getattr(eng, "devices", [0])))
            res["theta_search_lanes"] = ("lane i of a lockstep round on device i mod G (gpbo_group_lml_batch)" +
                                         ("" if distinct > 1 else "; virtual ranks on ONE physical GPU here: the gain of "
                                          "spreading the lanes is unmeasured on hardware"))
        res["default_call_is"] = ("suggest(n_random=M, n_smart=10, fit_gp=True) with GaussianProcessRegressor(Matern(2.5), alpha=1e-6, "
                                  "normalize_y=True, n_restarts_optimizer=5): theta search (LML + gradient on the device, lockstep "
                                  "restarts) + refit + M candidates + 10 local searches (gpbo_polish_seeds); median over 5 calls whose "
                                  "restarts start from RandomState(100..104) (per call: default_call_per_restart_seed; "
                                  "n_smart_10_with_theta_search uses the same seeds); default_call_interior = median over the calls whose "
                                  "search ran >= 10 lockstep rounds")
        # the same call on observations whose likelihood has its optimum in the interior FOR EVERY restart seed: the workload's X
        # with the smooth target of scripts/theta_search_timing.py, y = exp(-|x - 0.5|^2) + 0.01 noise (optimum near length scale
        # 1.2 at C2).  On the workload's own generator L-BFGS-B's first step from length scale 1 (gradient ~1e4 in log space, all
        # variables boxed: unit step) lands on the lower bound 1e-5 where the gradient is exactly 0 — scikit-learn itself ends
        # there unless a restart happens to start near the optimum (seeds 100 / 103) — so most calls time a 2-round search.
        rng2 = np.random.RandomState(0)
        y2 = np.exp(-((X - 0.5) ** 2).sum(1)) + 0.01 * rng2.standard_normal(len(X))
        sp2 = FloatSpace(w.pbounds())
        sp2.register_bulk(X, y2)
        lb = theta_block(sp2, "smooth")
        res["smooth_target"] = {"y": "exp(-sum((x - 0.5)^2)) + 0.01 * RandomState(0).standard_normal(N) on the workload's X",
                                **{k: lb[k] for k in ("default_call", "default_call_max", "default_call_interior",
                                                      "default_call_interior_n", "default_call_per_restart_seed")}}
    except Exception as e:  # noqa: BLE001
        res.setdefault("n_smart_10_with_theta_search", None)
        res["theta_search_error"] = repr(e)
    return res


def suggest_fixed_total(w, X, eng, M_total, n_gpus, mode):
    """The strong-scaling half of BASELINE.json's metric ("ms/suggest at N=4096 d=16, 1/2/4/8 GPUs"): THE SAME suggest() — the job's
    candidates fixed at M_total (2^20 for C3 / C4) however many GPUs share them — where `suggest_ms` above grows the job with the
    GPUs (n_random = M x n_gpus).  Two calls through the seams (FloatSpace + HipGPR + fused acquisition, as accelerate(optimizer,
    devices=[...]) installs them): fixed theta with n_smart = 0, and the reference's default call (theta search with 5 restarts in
    the fit + 10 local searches) on the smooth target, whose every restart seed ends at an interior optimum.  What does not shard
    is quoted by name: `theta_search_ms` (the fit incl. its search: replicated, or its lanes spread over the group),
    `posterior_ms_max_device` (the slowest device's posterior pass of the last call: the part that shrinks with 1/G) and
    `serial_fraction` = 1 - posterior_ms_max_device / default_call_ms.  Reference: bayes_opt/bayesian_optimization.py:323-333."""
    import warnings

    from sklearn.gaussian_process.kernels import Matern, RBF

    from bayesianoptimization_amd import fused_acquisition as A
    from bayesianoptimization_amd.float_space import FloatSpace
    from bayesianoptimization_amd.gpr import HipGPR

    def post_max():
        try:
            if mode == "group":
                return float(max(t["posterior_main"] for t in eng.per_device_timings()))
            return float(eng.last_timings()["posterior_main"])
        except Exception:  # noqa: BLE001
            return None

    fn = {W.UCB: lambda: A.UpperConfidenceBound(kappa=w.acq_param), W.EI: lambda: A.ExpectedImprovement(xi=w.acq_param),
          W.POI: lambda: A.ProbabilityOfImprovement(xi=w.acq_param)}[w.acq]()
    rng2 = np.random.RandomState(0)
    y2 = np.exp(-((X - 0.5) ** 2).sum(1)) + 0.01 * rng2.standard_normal(len(X))
    sp = FloatSpace(w.pbounds())
    sp.register_bulk(X, y2)
    kern = Matern(nu=2.5, length_scale=w.length_scale) if w.kernel == W.MATERN25 else RBF(length_scale=w.length_scale)
    out = {"n_random_total": int(M_total), "n_gpus": int(n_gpus), "scaling": "strong",
           "target": "smooth: exp(-sum((x - 0.5)^2)) + 0.01 * RandomState(0).standard_normal(N) on the workload's X"}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = HipGPR(kernel=kern, alpha=w.noise, normalize_y=True, optimizer=None, engine=eng, incremental=False)
        fn.device_polish = False
        ts = []
        for rep in range(4):
            t0 = time.perf_counter()
            fn.suggest(gp, sp, n_random=M_total, n_smart=0, fit_gp=True, random_state=np.random.RandomState(7 + rep))
            ts.append((time.perf_counter() - t0) * 1e3)
        out["fixed_theta_n_smart_0_ms"] = float(np.median(ts[1:]))
        out["fixed_theta_posterior_ms_max_device"] = post_max()
        gp_t = HipGPR(kernel=Matern(nu=2.5), alpha=1e-6, normalize_y=True, n_restarts_optimizer=5,
                      random_state=np.random.RandomState(1), engine=eng, incremental=False)
        fit0, fits = gp_t.fit, []

        def timed_fit(X_, y_):
            t0 = time.perf_counter()
            r = fit0(X_, y_)
            fits.append(((time.perf_counter() - t0) * 1e3, int(getattr(gp_t, "theta_search_rounds_", 0))))
            return r

        gp_t.fit = timed_fit
        fn.device_polish = "auto"
        ts = []
        for r, seed in enumerate((100, 100, 101, 102)):
            gp_t.random_state = np.random.RandomState(seed)
            t0 = time.perf_counter()
            fn.suggest(gp_t, sp, n_random=M_total, n_smart=10, fit_gp=True, random_state=np.random.RandomState(7 + r))
            ts.append((time.perf_counter() - t0) * 1e3)
        fn.device_polish = False
    out["default_call_ms"] = float(np.median(ts[1:]))
    out["theta_search_ms"] = float(np.median([f[0] for f in fits[1:]]))
    out["theta_search_rounds"] = [f[1] for f in fits[1:]]
    out["posterior_ms_max_device"] = post_max()
    if out["posterior_ms_max_device"]:
        out["serial_fraction"] = 1.0 - out["posterior_ms_max_device"] / out["default_call_ms"]
    if getattr(eng, "last_lane_devices", None) is not None:
        out["theta_search_lane_devices_last_round"] = list(eng.last_lane_devices)
    return out


def summary_of(out):
    """<= 1.5 KB digest, printed as the LAST key of the line: the driver's record keeps the headline keys and a tail of the
    line, and the per-seed tables of suggest_ms are long — the small configs' numbers used to fall off the front."""
    def r(v, n=4):
        return None if v is None else (round(float(v), n) if isinstance(v, (int, float)) else v)

    sm = {}
    for key, c_ in (out.get("configs") or {}).items():
        if "error" in c_:
            sm[key] = {"error": c_["error"][:60]}
            continue
        par = c_.get("parity") or {}
        sm[key] = {"ms": r(c_.get("ms_per_step")), "fit_ms": r(c_.get("fit_ms")), "frac": r(c_["roofline"]["frac"]),
                   "frac_step": r(c_["roofline"]["frac_of_whole_step"]),
                   "argmin_ok": par.get("argmin_equals_reference"), "top10_ok": par.get("top10_equals_reference")}
        sg = c_.get("suggest_ms") or {}
        if sg and "error" not in sg:
            sm[key]["suggest"] = {"n_smart_0": r(sg.get("n_smart_0"), 3), "default_interior": r(sg.get("default_call_interior"), 3),
                                  "default_smooth": r((sg.get("smooth_target") or {}).get("default_call"), 3)}
    sg = out.get("suggest_ms") or {}
    head = {"ms": r(out.get("ms_per_step")), "frac": r(out["roofline"]["frac"]), "fit_ms": r(out["roofline_fit"].get("fit_ms_per_gp")),
            "chol_ms": r(out["roofline_fit"].get("chol_ms")),
            "argmin_ok": (out.get("parity") or {}).get("argmin_equals_reference"),
            "top10_ok": (out.get("parity") or {}).get("top10_equals_reference")}
    if sg and "error" not in sg:
        head["suggest"] = {"n_smart_0": r(sg.get("n_smart_0"), 3), "default_interior": r(sg.get("default_call_interior"), 3),
                           "default_interior_minus_n_smart_0": r(sg.get("default_call_interior_minus_n_smart_0"), 3),
                           "default_smooth": r((sg.get("smooth_target") or {}).get("default_call"), 3)}
    ft = out.get("suggest_ms_fixed_total") or {}
    if ft and "error" not in ft:
        head["fixed_total"] = {k_: r(ft.get(k_), 3) for k_ in ("fixed_theta_n_smart_0_ms", "default_call_ms", "theta_search_ms",
                                                              "posterior_ms_max_device", "serial_fraction")}
    sm[out["config"]["workload"].split(":")[0]] = head
    sm["n_gpus"] = out.get("n_gpus")
    sm["cpu"] = r((out.get("cpu_baseline") or {}).get("value"), 1)
    return sm


def reference_golden(name, n_shards, M_shard):
    """The reference's answer for the job this run evaluates, from the committed goldens (tests/golden/, generated by
    oracle/gen_golden*.py driving bayes_opt itself): C3 -> C3.npz; C4/C5 at n_shards GPUs -> shards 0..n-1 merged as the
    reference would see the concatenated candidate matrix (argmin = first minimum, argsort = stable order)."""
    gdir = os.path.join(ROOT, "tests", "golden")
    if name not in SHARDED:
        p = os.path.join(gdir, f"{name}.npz")
        if n_shards != 1 or not os.path.exists(p):
            return None
        g = np.load(p)
        if int(g["M_evaluated"]) != M_shard:
            return None
        return {"argmin": int(g["argmin"]), "min": float(g["min"]), "top_idx": g["topk_idx"].astype(np.int64),
                "top_val": g["topk_val"], "source": f"tests/golden/{name}.npz"}
    vals, idxs = [], []
    for r in range(n_shards):
        p = os.path.join(gdir, f"{name}_s{r}.npz")
        if not os.path.exists(p):
            return None
        g = np.load(p)
        if int(g["M_evaluated"]) != M_shard or int(g["n_nan"]) != 0:
            return None
        vals.append(g["topk_val"])
        idxs.append(g["topk_idx"].astype(np.int64) + r * M_shard)
    vals, idxs = np.concatenate(vals), np.concatenate(idxs)
    o = np.lexsort((idxs, vals))
    return {"argmin": int(idxs[o[0]]), "min": float(vals[o[0]]), "top_idx": idxs[o], "top_val": vals[o],
            "source": f"tests/golden/{name}_s0..s{n_shards - 1}.npz (merged)"}


def measured_peak(eng, prec):
    """the spec peak AND the micro-benchmarked one.  ~0.2 s of device time: v_mfma_f64_16x16x4_f64 streams
    (gpbo_mfma_f64_probe, in-kernel s_memtime / s_memrealtime clocks) in the posterior GEMM's register pattern at 4 waves
    per SIMD and in the plain 8-accumulator pattern at 2 — `peak_measured` is the best of them, `sustained_mhz` the shader
    clock under that load, `peak_at_sustained_clock` = the device's CUs (256) x 4 SIMDs x 32 flop/clk x that clock (what the datasheet's
    78.6 TFLOP/s becomes at the clock this box holds; the fp32 matrix rate is twice that)."""
    probes = []
    for waves, mode in ((4, 2), (2, 0), (4, 0)):
        r = eng.mfma_f64_probe(iters=6000, waves_per_simd=waves, mode=mode)
        probes.append({"waves_per_simd": waves, "pattern": {0: "8 accumulators, one operand pair", 2: "2x4 tiles, six operand registers"}[mode],
                       "tflops_over_kernel_span": float(r["tflops"]), "shader_mhz": float(r["shader_mhz"]), "event_ms": float(r["ms"])})
    best = max(probes, key=lambda p: p["tflops_over_kernel_span"])
    scale = 2.0 if prec else 1.0
    try:
        cus = int(eng.device_info()["compute_units"])      # (hipDeviceProp.multiProcessorCount: 256 on an MI355X)
    except Exception:  # noqa: BLE001
        cus = 256
    return {"peak_measured": best["tflops_over_kernel_span"] * scale, "sustained_mhz": best["shader_mhz"], "compute_units": cus,
            "peak_at_sustained_clock": cus * 4 * 32 * best["shader_mhz"] * 1e6 / 1e12 * scale,
            "peak_measured_note": ("best of the v_mfma_f64_16x16x4_f64 micro-benchmarks below" + (" x 2 (fp32 matrix rate)" if prec else "")
                                   + "; a register-constant MFMA stream is not a ceiling for a kernel (docs/LAB_NOTEBOOK.md §4.1 fact 3): "
                                     "frac_of_measured may exceed what frac_at_sustained_clock allows"),
            "mfma_probes": probes}


def pmc_summary_for(w):
    """HBM-side bytes per launch of the dominant kernels from the rocprofv3 --pmc passes of THIS command
    (scripts/profile_pmc.sh -> scripts/pmc_summary.py), trusted only when the summary was taken from the very kernel
    sources this run uses (the library's build fingerprint is stamped into the summary)."""
    from bayesianoptimization_amd.build import _fingerprint
    # C4 is C3's GP over the same 2^20 candidates per GPU with another acquisition function: its dominant kernels
    # (and their launches) are the ones profiled for C3
    cfg = 'C3' if w.name == 'C4' else w.name
    cands = sorted((p for p in os.listdir(os.path.join(ROOT, "profiles")) if p.endswith(f"_pmc_{cfg}.json")), reverse=True)
    if not cands:
        return None, "no PMC summary for this config under profiles/ (scripts/profile_pmc.sh)"
    ppath = os.path.join(ROOT, "profiles", cands[0])       # the latest round's
    pm = json.load(open(ppath))
    meta = pm.get("_meta", {})
    if meta.get("source_fingerprint") != _fingerprint():
        return None, (f"profiles/{os.path.basename(ppath)} was taken at another state of the kernel sources "
                      f"(fingerprint {str(meta.get('source_fingerprint'))[:12]} != {_fingerprint()[:12]}): not reported")
    return pm, f"profiles/{os.path.basename(ppath)} (same kernel sources: fingerprint {_fingerprint()[:12]})"


def resolved(w):
    """Workloads whose theta comes from the reference's own fit (C1, F1: length_scale=None) read it from their golden file."""
    if w.length_scale is not None:
        return w
    import dataclasses
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{w.name}.npz"))
    return dataclasses.replace(w, length_scale=float(np.atleast_1d(g["length_scale"])[0]))


def run_extra_config(eng, name, steps=5, warmup=2, cpu_chunks=0):
    """One more BASELINE.json config on the already-open single engine, after the headline's timed region: the same step
    (fit at fixed theta + posterior + acquisition + arg-best/top-10 over the resident candidates; sharded configs: shard 0
    = one GPU's share of the 8-GPU job), every step wall-clocked by itself (median quoted, mean and max beside it), with the
    dominant kernels' HIP-event time and the parity block against the reference's golden for exactly this job.
    cpu_chunks > 0: the CPU path beside it (cpu_baseline on that many chunks of the same candidates)."""
    w = resolved(W.ALL[name])
    X, y, c = W.make_observations(w)
    y_mean, y_std = float(np.mean(y)), float(np.std(y))
    yn = (y - y_mean) / y_std
    y_max = W.feasible_y_max(w, y, c)
    M = w.M // 8 if w.name in SHARDED else w.M
    prec = 1 if w.dtype == "f32" else 0
    n_gp = 2 if w.constrained else 1
    lb_c = ub_c = None
    if w.constrained:
        c_mean, c_std = float(np.mean(c)), float(np.std(c))
        cn = (c - c_mean) / c_std
        lb_c, ub_c = [-np.inf], [w.constraint_ub]
    Xc = W.make_candidates(w.bounds_array(), M, 7)
    eng.set_candidates(Xc)
    post = [0.0]
    events = [False]
    # The steps are clocked with the calls NOT recording their HIP event pairs (gpbo_set_timing 0 — what the seams' shared engine
    # runs with: a record is a marker packet on the stream, and the eight of a step are 28 us of config 1's 119); a second pass of
    # the same steps with the records on gives the kernels' own times (posterior_ms, fit_ms) and is quoted beside the first.
    eng.set_timing(False)

    def step():
        if w.constrained:
            with eng.overlapped_fits():
                eng.fit(X, yn, w.kernel, w.length_scale, w.noise, slot=0, precision=prec)
                eng.fit(X, cn, W.MATERN25, w.constraint_length_scale, w.noise, slot=1, precision=prec)
        else:
            eng.fit(X, yn, w.kernel, w.length_scale, w.noise, slot=0, precision=prec)
        eng.posterior(0, y_mean, y_std, fetch=False)
        if w.constrained:
            # the two posteriors share one event pair: in the events pass the first is read (a stream synchronisation) before
            # the second is enqueued
            if events[0]:
                post[0] = eng.last_timings()["posterior_main"]
            eng.posterior(1, c_mean, c_std, fetch=False)
            if events[0]:
                post[0] += eng.last_timings()["posterior_main"]
        best = eng.acq_argbest(w.acq, w.acq_param, 0.0 if y_max is None else y_max, lb_c, ub_c, k_seeds=10)[:4]
        return best

    # Warm-up by TIME as well as by count: this block follows a CPU leg (seconds of host work with the GPU idle), and the first
    # milliseconds of GPU work after an idle spell run at ramping clocks — a 0.8 ms step timed over five steps right behind it was
    # once quoted at 4.9 ms (posterior kernel 4.4 instead of 0.37 ms; profiles/r04_bench_default_C3_with_configs.json's first run).
    # Short steps are also timed over more of them (>= 40 ms of work, at most 200 steps).
    t_w, warm = time.perf_counter(), []
    while len(warm) < warmup or time.perf_counter() - t_w < 0.06:
        t1 = time.perf_counter()
        step()
        eng.synchronize()
        warm.append(time.perf_counter() - t1)
    steps = max(steps, min(200, int(np.ceil(0.04 / max(float(np.median(warm)), 1e-5)))))
    # every step is clocked by itself (it ends in the read-back of the arg-best records, a stream synchronisation) and the MEDIAN
    # is quoted beside the mean: over ~50-200 sub-millisecond steps one stall of tens of milliseconds (seen twice behind the CPU legs
    # on the GPU box: once inside a posterior kernel, once outside) would otherwise be the number
    per_step, per_step_ev, per_post, per_fit = [], [], [], []
    for _ in range(steps):
        t1 = time.perf_counter()
        best = step()
        eng.synchronize()
        per_step.append((time.perf_counter() - t1) * 1e3)
    eng.set_timing(True)
    events[0] = True
    for i in range(2 + min(steps, 40)):
        t1 = time.perf_counter()
        step()
        eng.synchronize()
        if i < 2:
            continue
        per_step_ev.append((time.perf_counter() - t1) * 1e3)
        tl = eng.last_timings()
        per_post.append(post[0] if w.constrained else tl["posterior_main"])
        per_fit.append(tl["fit"])
    ms = float(np.median(per_step))
    main_ms = float(np.median(per_post))
    fit_ms = float(np.median(per_fit)) * steps
    fl = flops_per_candidate(w.N, w.d, n_gp) * M
    peak = FP32_MFMA_PEAK_TFLOPS if prec else FP64_MFMA_PEAK_TFLOPS
    theta_note = ""
    if name == "C2":
        theta_note = (f", FIXED length_scale={w.length_scale} (SURVEY.md §8(d) asks for the sklearn-fitted value at N <= 512: on this "
                      "generator sklearn's own search ends at the lower bound 1e-5, K = I — workloads.py; fitted theta: golden F1)")
    elif w.length_scale is not None:
        theta_note = f", fixed length_scale={w.length_scale}"
    out = {"workload": f"{w.name}{' shard 0 of 8' if w.name in SHARDED else ''}: d={w.d} N={w.N} {W.ACQ_NAMES[w.acq]} M={M}, {n_gp} GP(s){theta_note}",
           "dtype": "f32" if prec else "f64", "steps": steps, "ms_per_step": ms,
           "ms_per_step_is": "median of the steps, each clocked by itself, the calls not recording HIP event pairs (gpbo_set_timing 0, the seams' "
                             "setting); posterior_ms / fit_ms: the events of a second pass of the same steps",
           "ms_per_step_with_event_records": float(np.median(per_step_ev)),
           "ms_per_step_mean": float(np.mean(per_step)), "ms_per_step_max": float(np.max(per_step)),
           "value": M / (ms * 1e-3), "unit": "candidates/s",
           "roofline": {"bound": "mfma", "posterior_ms": main_ms, "achieved": fl / (main_ms * 1e-3) / 1e12, "peak": peak,
                        "unit": "TFLOP/s", "frac": fl / (main_ms * 1e-3) / 1e12 / peak,
                        "frac_of_whole_step": fl / (ms * 1e-3) / 1e12 / peak},
           "fit_ms": (fit_ms / steps) if not w.constrained else None}
    g = reference_golden(w.name, 1, M)
    if g is not None:
        top10 = np.asarray(best[2], dtype=np.int64)
        out["parity"] = {"argmin_equals_reference": bool(int(best[0]) == g["argmin"]),
                         "top10_equals_reference": bool(np.array_equal(top10, g["top_idx"][:10])),
                         "min_rel_err": float(abs(best[1] - g["min"]) / abs(g["min"])), "reference": g["source"],
                         "arithmetic": "fp32 posterior vs the fp64 reference" if prec else "fp64"}
    if cpu_chunks > 0:
        try:
            _, _, _, _, gpu_ys = eng.acq_argbest(w.acq, w.acq_param, 0.0 if y_max is None else y_max, lb_c, ub_c, k_seeds=0,
                                                 return_values=True)
            out["cpu_baseline"] = cpu_baseline(w, X, y, c, Xc, y_max, gpu_ys, n_chunks=cpu_chunks)
        except Exception as e:  # noqa: BLE001
            out["cpu_baseline"] = {"error": repr(e)}
    if name == "C2":      # the small config is where ms/suggest is a latency, not a throughput, number
        try:
            out["suggest_ms"] = suggest_latency(w, X, y, eng, M)
        except Exception as e:  # noqa: BLE001
            out["suggest_ms"] = {"error": repr(e)}
    return out


def suggest_in_child(n_gpus, config, timeout_s=100):
    """`python bench.py --gpus N --suggest-only` in a fresh process without the launcher's RANK/WORLD_SIZE environment."""
    import subprocess
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK", "MASTER_ADDR", "MASTER_PORT",
                        "TORCHELASTIC_RUN_ID", "GPBO_BENCH_DEVICE")}
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--gpus", str(n_gpus), "--config", config, "--suggest-only"],
                           env=env, capture_output=True, text=True, timeout=timeout_s)
        for line in p.stdout.splitlines():
            if line.startswith("{"):
                return json.loads(line)
        return {"error": f"child rc={p.returncode}: {p.stderr[-300:]}"}
    except Exception as e:  # noqa: BLE001
        return {"error": repr(e)}


def emit_failed(args, n_gpus, why):
    print(json.dumps({"metric": METRIC, "value": None, "unit": "candidates/s", "n_gpus": n_gpus, "steps": args.steps,
                      "warmup": args.warmup, "ms_per_step": None, "higher_is_better": True, "scaling": "weak",
                      "vs_baseline": None, "dtype": None, "data": "synthetic",
                      "config": {"workload": args.config or "C4", "collective": "FAILED"}, "error": why}), flush=True)


DUMP_MAX_VALUES = 1 << 20   # acquisition values written whole up to this many (8 MB), a fixed sample of this size beyond


def dump_outputs(d, best, ys=None):
    """--dump-outputs: the timed path's answer of its last step as float64 .npy files, so that two builds can be compared
    output for output (the inputs depend on the arguments alone).  best = (index, value, top-k indices, top-k values) as a
    caller of the arg-best receives it; ys = the acquisition value of every candidate (a seeded sample of a larger set,
    with the candidate indices it holds)."""
    os.makedirs(d, exist_ok=True)
    arrays = {"best_index": np.array([best[0]], dtype=np.float64), "best_value": np.array([best[1]], dtype=np.float64),
              "topk_index": np.asarray(best[2], dtype=np.float64), "topk_value": np.asarray(best[3], dtype=np.float64)}
    if ys is not None:
        ys = np.asarray(ys, dtype=np.float64)
        if ys.size > DUMP_MAX_VALUES:
            idx = np.sort(np.random.RandomState(0).choice(ys.size, DUMP_MAX_VALUES, replace=False))
            arrays["acq_values_index"] = idx.astype(np.float64)
            ys = ys[idx]
        arrays["acq_values"] = ys
    for name, a in arrays.items():
        np.save(os.path.join(d, f"{name}.npy"), a)
    log(f"[bench] wrote {', '.join(sorted(arrays))} to {d}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default=None,
                    help="BASELINE.json config; default: C3 on one GPU, C4 (= C3's GP with EI, 2^20 candidates per GPU, "
                         "8 x 2^20 at --gpus 8) when sharded")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also measure what the headline does not need: measured peak, PMC traffic, "
                         "parity with the reference, CPU baseline, the other BASELINE.json configs, ms/suggest")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(with --full) skip the CPU baseline")
    ap.add_argument("--no-suggest", action="store_true", help="(with --full) skip the ms/suggest measurement after the timed region")
    ap.add_argument("--suggest-only", action="store_true", help="(child of a multi-rank run) print only the suggest_ms object")
    ap.add_argument("--no-extra-configs", action="store_true",
                    help="(with --full) skip the other BASELINE.json configs (C2, C4 shard 0, C5 fp32 shard 0) run after the "
                         "default headline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    # collectives wait with a deadline (comm.hip); the closing barrier of a multi-rank run has to outlast rank 0's child process
    os.environ.setdefault("GPBO_COMM_TIMEOUT_S", "300")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and world != args.gpus:
        log(f"[bench] WORLD_SIZE={world} but --gpus {args.gpus}: using WORLD_SIZE")
    mode = "ranks" if world > 1 else ("group" if args.gpus > 1 else "single")
    n_gpus = world if mode == "ranks" else args.gpus

    w = resolved(W.ALL[args.config or ("C3" if n_gpus == 1 else "C4")])
    X, y, c = W.make_observations(w)
    y_mean, y_std = float(np.mean(y)), float(np.std(y))
    yn = (y - y_mean) / y_std
    y_max = W.feasible_y_max(w, y, c)
    # per-GPU candidate count: C3 = its own M; C4/C5 are quoted as 8-GPU jobs -> one eighth per GPU (weak scaling)
    M = w.M // 8 if w.name in SHARDED else w.M
    prec = 1 if w.dtype == "f32" else 0
    n_gp = 2 if w.constrained else 1
    if w.constrained:
        c_mean, c_std = float(np.mean(c)), float(np.std(c))
        cn = (c - c_mean) / c_std
        lb_c, ub_c = [-np.inf], [w.constraint_ub]
    else:
        lb_c = ub_c = None

    # ---- devices and the exchange ---------------------------------------------------------------------------------
    collective = "none"
    if mode == "group":
        # GPBO_BENCH_DEVICES=0,0 rehearses the sharded flow with virtual ranks on one GPU
        devs = [int(t) for t in os.environ["GPBO_BENCH_DEVICES"].split(",")] if os.environ.get("GPBO_BENCH_DEVICES") \
            else list(range(n_gpus))
        try:
            eng = GroupEngine(devs)
        except Exception as e:  # noqa: BLE001
            emit_failed(args, n_gpus, f"device group: {e!r}")
            sys.exit(2)
        collective = eng.collective
        Xc = np.concatenate([W.make_candidates(w.bounds_array(), M, 7 + r) for r in range(n_gpus)])   # shard r -> device r
        eng.set_candidates(Xc)
        argbest = lambda: eng.acq_argbest(w.acq, w.acq_param, 0.0 if y_max is None else y_max, lb_c, ub_c, k_seeds=10)[:4]  # noqa: E731
        barrier_max = lambda v: (eng.synchronize(), v)[1]  # noqa: E731
    else:
        dev = int(os.environ.get("GPBO_BENCH_DEVICE", local_rank))
        try:
            eng = GpEngine(dev)
        except Exception as e:  # noqa: BLE001
            why = f"rank {rank}: no usable device {dev} ({e!r}); --gpus {n_gpus} needs {n_gpus} GPUs on this node"
            log(f"[bench] {why}")
            if rank == 0:
                emit_failed(args, n_gpus, why)
            sys.stdout.flush()
            sys.exit(3)
        if mode == "ranks":
            state = {"ok": False, "err": None}

            def _init():
                try:
                    uid = rendezvous.share_unique_id(rank, GpEngine.comm_unique_id)
                    eng.comm_init(uid, world, rank)
                    state["ok"] = True
                except Exception as e:  # noqa: BLE001
                    state["err"] = repr(e)

            th = threading.Thread(target=_init, daemon=True)
            th.start()
            th.join(timeout=float(os.environ.get("GPBO_RCCL_INIT_TIMEOUT", "300")))
            if not state["ok"]:
                why = f"RCCL bootstrap failed or hung on rank {rank}: {state['err']}"
                log(f"[bench] {why}")
                if rank == 0:
                    emit_failed(args, n_gpus, why)
                sys.stdout.flush()
                os._exit(3)        # a hung ncclCommInitRank thread must not keep the process alive
            collective = "rccl-allgather"
        Xc = W.make_candidates(w.bounds_array(), M, 7 + rank)  # rank r: shard r of a weak-scaled candidate set
        sh = ShardedAcquisition(eng, world, rank)
        sh.set_candidates_local(Xc, offset=rank * M)
        argbest = lambda: sh.argbest(w.acq, w.acq_param, 0.0 if y_max is None else y_max, lb_c, ub_c, k_seeds=10)  # noqa: E731
        barrier_max = (lambda v: eng.comm_allreduce_max(v)) if mode == "ranks" else (lambda v: (eng.synchronize(), v)[1])

    if args.suggest_only:
        res = suggest_latency(w, X, y, eng, M * n_gpus)
        res["engine"] = (f"GroupEngine over {n_gpus} device(s) ({collective})" if mode == "group" else "GpEngine") + f", n_random = {M * n_gpus}"
        try:
            res["fixed_total"] = suggest_fixed_total(w, X, eng, M, n_gpus, mode)
        except Exception as e:  # noqa: BLE001
            res["fixed_total"] = {"error": repr(e)}
        print(json.dumps(res), flush=True)
        eng.close()
        return

    post_ms = [0.0]
    fits_ms = [0.0]
    # the target GP's and the constraint GP's factorisations of one step are independent: enqueued side by side
    # (GpEngine.overlapped_fits -> gpbo_fit_begin / gpbo_fit_wait), as the fused acquisition's _fit_gp does
    overlap = w.constrained and hasattr(eng, "overlapped_fits") and os.environ.get("GPBO_BENCH_OVERLAP_FITS", "1") != "0"

    def step():
        if overlap:
            t_f = time.perf_counter()
            with eng.overlapped_fits():
                eng.fit(X, yn, w.kernel, w.length_scale, w.noise, slot=0, precision=prec)
                eng.fit(X, cn, W.MATERN25, w.constraint_length_scale, w.noise, slot=1, precision=prec)
            fits_ms[0] = (time.perf_counter() - t_f) * 1e3
            eng.posterior(0, y_mean, y_std, fetch=False)
            post_ms[0] = eng.last_timings()["posterior_main"]
            eng.posterior(1, c_mean, c_std, fetch=False)
            post_ms[0] += eng.last_timings()["posterior_main"]
            return argbest()
        eng.fit(X, yn, w.kernel, w.length_scale, w.noise, slot=0, precision=prec)
        eng.posterior(0, y_mean, y_std, fetch=False)
        if w.constrained:   # constraint GP in slot 1 (bayes_opt/constraint.py:132-151, 199-221)
            # the two posteriors share one event pair: the first is read (a stream synchronisation) before the second is enqueued
            post_ms[0] = eng.last_timings()["posterior_main"]
            eng.fit(X, cn, W.MATERN25, w.constraint_length_scale, w.noise, slot=1, precision=prec)
            eng.posterior(1, c_mean, c_std, fetch=False)
            post_ms[0] += eng.last_timings()["posterior_main"]
        best = argbest()
        if not w.constrained:
            post_ms[0] = eng.last_timings()["posterior_main"]   # after the step: the harness puts no synchronisation inside it
        return best

    for _ in range(args.warmup):
        step()
    fit_probe = None
    if overlap and args.full:
        # stage timings of ONE fit on the main stream (the overlapped fits are not bracketed by the timing events); outside
        # the timed region.  A plain run has no fit stage timings to quote (null in the line)
        eng.fit(X, yn, w.kernel, w.length_scale, w.noise, slot=0, precision=prec)
        fit_probe = dict(eng.last_timings())
    kern_ms = {"fit": 0.0, "posterior_main": 0.0, "posterior_finalize": 0.0, "acq_argbest": 0.0, "kmat": 0.0,
               "cholesky": 0.0, "trtri": 0.0}
    kern_ms_overlapped = [0.0]
    barrier_max(0.0)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        best = step()
        tm = dict(eng.last_timings())  # HIP events recorded on the (first) engine's own stream around each kernel group
        if fit_probe is not None:
            for k_ in ("fit", "kmat", "cholesky", "trtri"):
                tm[k_] = fit_probe[k_]
        for k_ in kern_ms:
            kern_ms[k_] += tm[k_] * (n_gp if k_ in ("fit", "kmat", "cholesky", "trtri") else 1)
        kern_ms_overlapped[0] += fits_ms[0]
        kern_ms["posterior_main"] += post_ms[0] - tm["posterior_main"]   # both GPs' posterior launches
    barrier_max(0.0)
    elapsed = barrier_max(time.perf_counter() - t0)
    if args.dump_outputs and rank == 0:
        ys = None
        if mode != "ranks":   # the acquisition values behind that arg-best, read back outside the timed region
            ys = eng.acq_argbest(w.acq, w.acq_param, 0.0 if y_max is None else y_max, lb_c, ub_c, k_seeds=0,
                                 return_values=True)[4]
        dump_outputs(args.dump_outputs, best, ys)
    per_rank = None
    if mode == "ranks":
        # every rank's stage times of its last step, gathered as (value, rank) records over the same RCCL communicator
        tl = eng.last_timings()
        try:
            av, ai = eng.comm_allgather_best(np.array([tl["fit"], tl["posterior_main"], tl["acq_argbest"]]),
                                             np.full(3, rank, dtype=np.int64))
            av, ai = np.asarray(av).reshape(world, 3), np.asarray(ai).reshape(world, 3)
            per_rank = [{"rank": int(ai[r, 0]), "fit": float(av[r, 0]), "posterior_main": float(av[r, 1]), "acq_argbest": float(av[r, 2])}
                        for r in range(world)]
        except Exception as e:  # noqa: BLE001
            log(f"[bench] per-rank timings not gathered: {e!r}")

    # what the hardware and RCCL say about this run (PCI bus ids, ncclCommCount), gathered before rank 0 prints: a first run on
    # more than one physical GPU judges itself from the line
    hw = {"rccl_nranks": None, "devices": None}
    code, nr = -1.0, -1.0          # this rank's PCI (domain, bus) as one number, and what ncclCommCount says
    try:
        if mode == "group":
            infos = eng.per_device_info()
            hw["devices"] = [i_["pci_bus_id"] for i_ in infos]
            hw["rccl_nranks"] = [i_["rccl_nranks"] for i_ in infos]
            hw["distinct_physical_gpus"] = len(set(hw["devices"]))
        else:
            info = eng.device_info()
            hw["devices"] = [info["pci_bus_id"]]
            hw["rccl_nranks"] = info["rccl_nranks"]
            bus = info["pci_bus_id"].split(":")
            if len(bus) >= 2:
                code = float(int(bus[0], 16) * 256 + int(bus[1], 16))
            nr = float(info["rccl_nranks"])
    except Exception as e:  # noqa: BLE001
        hw["error"] = repr(e)
    if mode == "ranks":
        # every rank enters this exchange whatever happened above (a rank that skipped it would leave its peers waiting for the
        # collective's deadline): (PCI domain:bus, ncclCommCount) of every rank as records over the same communicator
        try:
            av, _ = eng.comm_allgather_best(np.array([code, nr]), np.full(2, rank, dtype=np.int64))
            av = np.asarray(av).reshape(world, 2)
            hw["devices"] = [(f"{int(v) // 256:04x}:{int(v) % 256:02x}" if v >= 0 else "?") for v in av[:, 0]]
            hw["rccl_nranks"] = [int(v) for v in av[:, 1]]
            hw["distinct_physical_gpus"] = len(set(hw["devices"]))
        except Exception as e:  # noqa: BLE001
            hw["error"] = repr(e)

    if rank == 0:
        steps = args.steps
        ms_per_step = elapsed / steps * 1e3
        value = n_gpus * M * steps / elapsed
        main_ms = kern_ms["posterior_main"] / steps
        fl = flops_per_candidate(w.N, w.d, n_gp) * M
        achieved = fl / (main_ms * 1e-3) / 1e12
        peak = FP32_MFMA_PEAK_TFLOPS if prec else FP64_MFMA_PEAK_TFLOPS
        kmat_ms, chol_ms = kern_ms["kmat"] / steps / n_gp, kern_ms["cholesky"] / steps / n_gp
        NP = (w.N + 63) // 64 * 64
        kmat_bytes = NP * (NP + 64) / 2 * 8          # lower block triangle written once
        chol_flops = float(w.N) ** 3 / 3.0
        out = {
            "metric": METRIC,
            "value": value, "unit": "candidates/s", "n_gpus": n_gpus, "steps": steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32" if prec else "f64", "data": "synthetic",
            "config": {"workload": f"{w.name}: d={w.d} N={w.N} {W.KERNEL_NAMES[w.kernel]} {W.ACQ_NAMES[w.acq]} "
                                   f"M={M} candidates per GPU, {n_gp} GP(s), fixed length_scale={w.length_scale}, "
                                   f"alpha={w.noise}, k_seeds=10; BASELINE.json config {w.name}",
                       "N": w.N, "d": w.d, "M_per_gpu": M, "M_total": M * n_gpus, "collective": collective,
                       "rccl_nranks": hw["rccl_nranks"], "devices": hw["devices"],
                       "distinct_physical_gpus": hw.get("distinct_physical_gpus", 1),
                       "multi_gpu_measured_on_hardware": bool(hw.get("distinct_physical_gpus", 1) == n_gpus) if n_gpus > 1 else None,
                       "processes": ("one per GPU (ncclCommInitRank, file rendezvous)" if mode == "ranks" else
                                     "one for all GPUs (gpbo_group, ncclCommInitAll)" if mode == "group" else "one")},
            "roofline": {"bound": "mfma", "kernel": ("kstar_gen_f32_kernel + posterior_kernel_f32" if prec else
                                                     "kstar_gen_kernel + posterior_kernel_v2<GEN=2>") + " (k* slab + MFMA GEMM)",
                         "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                         "traffic": None, "avg_launch_ms": main_ms, "flops_per_launch_algorithmic": fl},
            # the fit path on its own rooflines (north_star: "achieved HBM GB/s on kernel assembly", "MFMA utilisation on
            # the Cholesky"); HIP events on the engine's stream around each group, averaged over the timed steps
            "roofline_fit": {"kmat_ms": kmat_ms, "kmat_GBps": kmat_bytes / (kmat_ms * 1e-3) / 1e9 if kmat_ms > 0 else None,
                             "kmat_frac_of_achievable_hbm": (kmat_bytes / (kmat_ms * 1e-3) / 1e12 / HBM_ACHIEVABLE_TBPS)
                             if kmat_ms > 0 else None,
                             "kmat_bytes_algorithmic": kmat_bytes,
                             "chol_ms": chol_ms, "chol_TFLOPs": chol_flops / (chol_ms * 1e-3) / 1e12 if chol_ms > 0 else None,
                             "chol_frac": (chol_flops / (chol_ms * 1e-3) / 1e12 / FP64_MFMA_PEAK_TFLOPS) if chol_ms > 0 else None,
                             "chol_flops_algorithmic": chol_flops, "fit_ms_per_gp": kern_ms["fit"] / steps / n_gp},
            "step_breakdown_ms": {k_: v / steps for k_, v in kern_ms.items()},
            "best": {"index": int(best[0]), "value": float(best[1])},
        }
        # per-device stage times of the LAST timed step (HIP events on each device's own stream): a straggler is visible here
        if mode == "group":
            out["per_device_ms"] = [{"device": dv, "fit": t["fit"], "posterior_main": t["posterior_main"], "acq_argbest": t["acq_argbest"]}
                                    for dv, t in zip(devs, eng.per_device_timings())]
        elif mode == "ranks":
            out["per_device_ms"] = per_rank
        if overlap:
            # `fit`, `kmat`, `cholesky`, `trtri` above = n_gp x ONE fit measured alone on the main stream; in the timed steps
            # the fits of the GPs run side by side:
            out["step_breakdown_ms"]["fits_overlapped_wall"] = kern_ms_overlapped[0] / steps
            if fit_probe is None:     # plain run: no fit was measured alone, and the overlapped fits carry no stage events
                out["step_breakdown_ms"].update({k_: None for k_ in ("fit", "kmat", "cholesky", "trtri")})
                out["roofline_fit"] = {"note": "the two GPs' fits run side by side: stage timings of one fit alone with --full"}
            else:
                out["roofline_fit"]["note"] = ("stage timings of one fit measured alone (outside the timed region); in the timed "
                                               "steps the two GPs' fits are enqueued side by side: "
                                               "step_breakdown_ms.fits_overlapped_wall")
        if args.full:
            if mode == "single":
                try:
                    mp = measured_peak(eng, prec)
                    out["roofline"].update(mp)
                    out["roofline"]["frac_of_measured"] = achieved / mp["peak_measured"]
                    out["roofline"]["frac_at_sustained_clock"] = achieved / mp["peak_at_sustained_clock"]
                except Exception as e:  # noqa: BLE001
                    log(f"[bench] measured peak not available: {e!r}")
            # HBM traffic of the dominant kernels: separate rocprofv3 --pmc passes of this very command, summarised in profiles/
            try:
                pm, note = pmc_summary_for(w)
                out["roofline"]["traffic_note"] = note
                if pm is not None:
                    keys = [k_ for k_ in pm if "posterior_kernel" in k_ or "kstar_gen" in k_]
                    out["roofline"]["traffic"] = sum(pm[k_].get("fetch_bytes_corrected_x2", 0.0) * pm[k_].get("launches_per_step", 1)
                                                     + pm[k_].get("write_bytes", 0.0) * pm[k_].get("launches_per_step", 1) for k_ in keys)
                    out["roofline"]["traffic_algorithmic"] = (w.d + 1) * 8 * M * n_gp + n_gp * w.N * w.N * 4
                    busy = [pm[k_].get("mfma_pipe_busy_frac") for k_ in keys
                            if "posterior_kernel" in k_ and pm[k_].get("mfma_pipe_busy_frac")]
                    out["roofline"]["mfma_pipe_busy_frac_pmc"] = max(busy) if busy else None
                    for k_ in pm:
                        if k_.startswith("_"):
                            continue
                        if "gemm128" in k_ and pm[k_].get("mfma_pipe_busy_frac") is not None:
                            out["roofline_fit"].setdefault("trailing_update_mfma_busy", {})[k_[:60]] = pm[k_]["mfma_pipe_busy_frac"]
            except Exception as e:  # noqa: BLE001
                log(f"[bench] PMC summary not usable: {e!r}")
            # parity with the reference's answer for exactly this job (any n_gpus)
            g = reference_golden(w.name, n_gpus, M)
            if g is not None:
                top10 = np.asarray(best[2], dtype=np.int64)
                out["parity"] = {"argmin_equals_reference": bool(int(best[0]) == g["argmin"]),
                                 "top10_equals_reference": bool(np.array_equal(top10, g["top_idx"][:10])),
                                 "argmin_in_reference_top16": bool(int(best[0]) in set(g["top_idx"][:16].tolist())),
                                 "min_rel_err": float(abs(best[1] - g["min"]) / abs(g["min"])),
                                 "reference": g["source"],
                                 "arithmetic": "fp32 posterior vs the fp64 reference" if prec else "fp64"}
            if mode == "single" and not args.no_cpu_baseline:
                try:
                    _, _, _, _, gpu_ys = eng.acq_argbest(w.acq, w.acq_param, 0.0 if y_max is None else y_max, lb_c, ub_c,
                                                         k_seeds=0, return_values=True)
                    out["cpu_baseline"] = cpu_baseline(w, X, y, c, Xc, y_max, gpu_ys)
                except Exception as e:
                    log(f"[bench] cpu_baseline failed: {e!r}")
                    out["cpu_baseline"] = None
            if mode == "single" and args.config is None and not args.no_extra_configs:
                # every other BASELINE.json config, in the line the driver records (5 steps each, the CPU path beside each on a
                # bounded sample: C1 / C2 whole or 3 chunks, the two big shards 2 chunks)
                out["configs"] = {}
                for key, nm, cpu_chunks in (("C1", "C1", 1), ("C2", "C2", 3), ("C4_s0", "C4", 2), ("C5_f32_s0", "C5", 2)):
                    try:
                        out["configs"][key] = run_extra_config(eng, nm, cpu_chunks=cpu_chunks)
                    except Exception as e:  # noqa: BLE001
                        log(f"[bench] extra config {key} failed: {e!r}")
                        out["configs"][key] = {"error": repr(e)}
                eng.set_candidates(Xc)
            if mode in ("single", "group") and not w.constrained and not args.no_suggest:
                # the other half of BASELINE.json's metric, ms/suggest: whole suggest() calls through the drop-in seams
                # (refit at fixed theta, candidates drawn from the caller's RandomState on the device, posterior, acquisition,
                # arg-best; with the reference's default 10 local searches and without) — outside the timed region above
                try:
                    # group mode: the same seams over the device group, as accelerate(optimizer, devices=[...]) installs it
                    # (one process, candidates sharded over the GPUs, n_random = the whole job's candidates)
                    out["suggest_ms"] = suggest_latency(w, X, y, eng, M * n_gpus)
                    if mode == "group":
                        out["suggest_ms"]["engine"] = f"GroupEngine over {n_gpus} device(s), n_random = {M * n_gpus}"
                except Exception as e:  # noqa: BLE001
                    log(f"[bench] suggest latency failed: {e!r}")
            if mode == "ranks" and not w.constrained and not args.no_suggest:
                # ms/suggest for the same N GPUs: BayesianOptimization.suggest() is ONE process (accelerate(devices=[...]) ->
                # GroupEngine), so rank 0 measures it in a child process that owns all N devices while the other ranks idle at
                # the closing barrier; a child that fails or exceeds its deadline costs only this key
                out["suggest_ms"] = suggest_in_child(n_gpus, w.name)
            if mode in ("single", "group") and not w.constrained and not args.no_suggest:
                # ... and the same suggest() with the job's candidates FIXED at the config's own M (2^20), however many GPUs share it
                try:
                    out["suggest_ms_fixed_total"] = suggest_fixed_total(w, X, eng, M, n_gpus, mode)
                except Exception as e:  # noqa: BLE001
                    out["suggest_ms_fixed_total"] = {"error": repr(e)}
            elif mode == "ranks" and isinstance(out.get("suggest_ms"), dict) and "fixed_total" in out["suggest_ms"]:
                out["suggest_ms_fixed_total"] = out["suggest_ms"].pop("fixed_total")
        try:
            out["summary"] = summary_of(out)       # LAST key: survives a record that keeps only the line's tail
        except Exception as e:  # noqa: BLE001
            out["summary"] = {"error": repr(e)}
        print(json.dumps(out), flush=True)
    if mode == "ranks":
        # the other ranks sleep on the HOST while rank 0 measures ms/suggest in its child process (their GPUs stay idle for
        # it: a collective entered now would spin on them), then everybody meets in one last collective
        rendezvous.mark_done(rank)
        if not rendezvous.wait_done(rank, timeout=float(os.environ.get("GPBO_BENCH_TAIL_TIMEOUT_S", "150"))):
            log(f"[bench] rank {rank}: rank 0 did not report the end of its tail; entering the closing barrier anyway")
        try:
            barrier_max(0.0)
        except Exception as e:  # noqa: BLE001  (a closing barrier that fails changes nothing that was measured)
            log(f"[bench] rank {rank}: closing barrier: {e!r}")
        rendezvous.cleanup(rank)
    eng.close()


if __name__ == "__main__":
    main()
