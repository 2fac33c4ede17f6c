"""TEST INFRASTRUCTURE — golden vectors for the opt-in scaled kernels (ConstantKernel * k + WhiteKernel), produced by THE REFERENCE ITSELF.

    python scripts/gen_scaled_kernel_golden.py [--reference DIR]

Runs only where the reference (bayes_opt 3.3.0, not installed, not part of this repository) can be imported: from DIR, from
$GPBO_REFERENCE_ROOT, or from wherever `import bayes_opt` finds it.  (The scripts do not import oracle/ — tests/test_abi.py — so the
two things oracle/refenv.py does for the tests are restated in `import_reference` below.)  It drives the real bayes_opt BayesianOptimization with
`set_gp_params(kernel=ConstantKernel() * Matern(nu=2.5) + WhiteKernel())` exactly as suggest() does
(bayesian_optimization.py:323-333 -> acquisition.py:116-169): the reference's TargetSpace, wrapped kernel, GaussianProcessRegressor,
`_fit_gp` (theta search included), `_get_acq` closure and `random_sample` produce every number stored.  Shape: d = 3, N = 60,
M = 4096.  Output: tests/golden/scaled_kernel.npz — data only: X, y, the candidates, the fitted theta (as constant_value, length
scale and noise_level), alpha_, mu, sd, -acq for UCB and EI, their arg-best and top-16, and the library versions.
tests/test_scaled_kernel_host.py pins it against scikit-learn on the CPU; tests/test_gpu_scaled_kernel.py runs the device's full
acquisition pass against it, fitting at the stored theta.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def import_reference(root=None):
    """`bayes_opt` from `root` (or the import path as it is), with the two allowances an uninstalled checkout needs: `colorama`
    (coloured log output only) may be absent, and bayes_opt/__init__.py asks importlib.metadata for its distribution's version."""
    import importlib
    import importlib.metadata as md
    import types

    if root:
        if not os.path.isdir(os.path.join(root, "bayes_opt")):
            raise ImportError(f"no bayes_opt under {root}")
        if root not in sys.path:
            sys.path.insert(0, root)
    try:
        importlib.import_module("colorama")
    except ImportError:
        class _Codes:
            def __getattr__(self, name):
                return ""

        stub = types.ModuleType("colorama")
        stub.Fore = stub.Back = stub.Style = _Codes()
        stub.just_fix_windows_console = stub.init = lambda *a, **k: None
        sys.modules["colorama"] = stub
    if not getattr(md.version, "_gpbo_patched", False):
        orig = md.version

        def version(name):
            return "3.3.0" if name == "bayesian-optimization" else orig(name)

        version._gpbo_patched = True
        md.version = version
    return importlib.import_module("bayes_opt")


OUT = os.path.join(ROOT, "tests", "golden", "scaled_kernel.npz")
D, N, M, TOPK = 3, 60, 4096, 16
DATA_SEED, CAND_SEED = 21, 7      # (the Matern family golden's data and candidates)
KAPPA, XI = 2.576, 0.01


def observations():
    rng = np.random.RandomState(DATA_SEED)
    X = rng.uniform(size=(N, D))
    y = np.sin(3 * X.sum(1)) + 0.1 * rng.randn(N)
    return X, y


def generate(X, y) -> dict:
    from bayes_opt import BayesianOptimization, acquisition
    from sklearn.gaussian_process.kernels import ConstantKernel, Matern, WhiteKernel

    out = {}
    Xc = None
    for name, fn in (("ucb", acquisition.UpperConfidenceBound(kappa=KAPPA)), ("ei", acquisition.ExpectedImprovement(xi=XI))):
        opt = BayesianOptimization(f=None, pbounds={f"x{t}": (0.0, 1.0) for t in range(D)}, acquisition_function=fn,
                                   random_state=np.random.RandomState(3), verbose=0, allow_duplicate_points=True)
        for i in range(N):
            opt.register(params=X[i], target=y[i])
        space, gp = opt._space, opt._gp
        assert np.array_equal(space.params, X) and np.array_equal(space.target, y)
        opt.set_gp_params(kernel=ConstantKernel() * Matern(nu=2.5) + WhiteKernel())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fn._fit_gp(gp, space)
            if name == "ei":
                fn.y_max = space._target_max()
            cand = space.random_sample(M, np.random.RandomState(CAND_SEED))
            ys = fn._get_acq(gp=gp, constraint=space.constraint)(cand)
            mu, sd = gp.predict(cand, return_std=True)
        if Xc is None:
            Xc = cand
            k = gp.kernel_      # Sum(Product(ConstantKernel, Matern), WhiteKernel)
            out.update({"constant_value": np.float64(k.k1.k1.constant_value), "noise_level": np.float64(k.k2.noise_level),
                        "length_scale": np.atleast_1d(k.k1.k2.length_scale).astype(np.float64), "theta": k.theta.copy(),
                        "alpha_estimator": np.float64(gp.alpha),
                        "y_mean": np.float64(gp._y_train_mean), "y_std": np.float64(gp._y_train_std), "alpha": gp.alpha_.copy(),
                        "mu": mu, "sd": sd, "y_max": np.float64(np.max(y))})
        else:      # the same seed, the same data: both policies saw one model and one candidate set
            assert np.array_equal(cand, Xc) and np.array_equal(mu, out["mu"]) and np.array_equal(sd, out["sd"])
        top = np.argsort(ys)[:TOPK].astype(np.int64)
        out.update({f"ys_{name}": ys, f"argmin_{name}": np.int64(ys.argmin()), f"topk_idx_{name}": top, f"topk_val_{name}": ys[top].copy()})
    return Xc, out


def main():
    import argparse

    import scipy
    import sklearn

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=os.environ.get("GPBO_REFERENCE_ROOT"), help="directory that holds the bayes_opt package")
    import_reference(ap.parse_args().reference)
    X, y = observations()
    blob = {"X": X, "y": y, "kappa": np.float64(KAPPA), "xi": np.float64(XI),
            "versions": np.array(["bayes_opt 3.3.0", "sklearn " + sklearn.__version__, "scipy " + scipy.__version__, "numpy " + np.__version__])}
    Xc, out = generate(X, y)
    blob["candidates"] = Xc
    blob.update(out)
    print(f"constant_value {out['constant_value']}, length scale {out['length_scale']}, noise_level {out['noise_level']}, "
          f"UCB argmin {int(out['argmin_ucb'])} (top-2 gap {out['topk_val_ucb'][1] - out['topk_val_ucb'][0]:.3e}), "
          f"EI argmin {int(out['argmin_ei'])} (top-2 gap {out['topk_val_ei'][1] - out['topk_val_ei'][0]:.3e})")
    np.savez_compressed(OUT, **blob)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
