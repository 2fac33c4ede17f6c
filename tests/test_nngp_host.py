"""CPU: nngp_truth against a dense exact GP at N == k; the reference's own fp64-versus-longdouble spread and the neighbour gap on every
case of tests/test_gpu_nngp.py; include/gpnn.h: C99, exported exactly, bound by _lib; suggest_local's argument checks and gates."""
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import batch_truth as B
import matern_family_truth as F
import nngp_truth as T
import test_gpu_nngp as GPU
from bayesianoptimization_amd import _lib, suggest_local
from bayesianoptimization_amd.localgp import ConstrainedSpaceNotImplemented
from conftest import ROOT
from helpers import FakeEngine

INCLUDE = os.path.join(ROOT, "include")


@pytest.mark.parametrize("kind", [F.RBF, F.MATERN25, F.MATERN15, F.MATERN05])
def test_the_truth_is_the_exact_gp_when_every_row_is_a_neighbour(kind):
    case = (32, 32, 65, 3, kind, T.UCB, None)
    X, yn, ls, Xc = GPU.inputs(*case)[:4]
    want = T.nngp(kind, X, yn, ls, GPU.ALPHA, Xc, 32, T.UCB, 2.0, 0.0, GPU.Y_MEAN, GPU.Y_STD)
    gp = F.fit_fixed_theta(kind, X, yn, ls, noise=GPU.ALPHA, normalize_y=False)
    mu, sd = F.predict(gp, Xc)
    assert np.array_equal(np.sort(want["nbr"], axis=1), np.tile(np.arange(32), (65, 1))) and want["gap"] == np.inf
    assert np.abs(want["mu"] - (GPU.Y_MEAN + GPU.Y_STD * mu)).max() <= 1e-10 and np.abs(want["sd"] - GPU.Y_STD * sd).max() <= 1e-9


@pytest.mark.parametrize("case", GPU.CASES, ids=GPU.IDS)
def test_the_truths_own_spread_and_the_neighbour_gap(case):
    want = GPU.truth(case)
    print(f"{case}: D {want['D']:.2e}, gap {want['gap']:.2e}")
    assert want["D"] <= 2.5e-10 and want["gap"] >= 1e-9 and GPU.ALPHA >= 1e-4
    assert np.isfinite(want["ys"].astype(np.float64)).all() and (want["sd"] > 0).all()


def test_the_header_is_c99_and_both_libraries_export_exactly_its_names(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no host C compiler")
    (tmp_path / "only.c").write_text('#include "gpnn.h"\nint main(void) { return GPNN_MAX_NEIGHBORS == 64 && GPNN_MAX_N == 1048576 ? 0 : 1; }\n')
    for flags in ([], ["-DGPBO_DEBUG"]):
        subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", *flags, "-I", INCLUDE,
                        str(tmp_path / "only.c")], check=True)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "gpnn.h")).read(), flags=re.S)
    head, rest = src.split("#ifdef GPBO_DEBUG", 1)
    product, debug = (sorted(set(re.findall(r"\b(gpnn_\w+)\s*\(", part))) for part in (head, rest.split("#endif", 1)[0]))
    assert product == ["gpnn_acq_argbest"] == sorted(_lib.NN_SIGNATURES) and debug == ["gpnn_debug_stage_ms"] == sorted(_lib.NN_DEBUG_SIGNATURES)
    assert _lib.MAX_NN_NEIGHBORS == 64 and _lib.MAX_NN_N == 1 << 20
    for path, names in ((_lib.LIB_PATH, product), (_lib.DEBUG_LIB_PATH, sorted(product + debug))):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert sorted({ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("gpnn")}) == names, path
    for name, table in (("gpnn_acq_argbest", _lib.NN_SIGNATURES), ("gpnn_debug_stage_ms", _lib.NN_DEBUG_SIGNATURES)):
        args = re.search(name + r"\s*\((.*?)\);", src, flags=re.S).group(1)
        assert len(args.split(",")) == len(table[name][1]), name


BAD = [(dict(n_neighbors=20), "n_neighbors"), (dict(n_neighbors=True), "n_neighbors"), (dict(n_neighbors=32.0), "n_neighbors"),
       (dict(n_random=0), "n_random"), (dict(n_random=1.5), "n_random"), (dict(theta_subset=31), "theta_subset"),
       (dict(theta_subset=65537), "theta_subset"), (dict(acquisition="pi"), "acquisition"), (dict(kappa=np.nan), "kappa"),
       (dict(acquisition="ei", xi=np.inf), "xi")]


@pytest.mark.parametrize("kw,match", BAD)
def test_suggest_local_argument_errors(kw, match):
    fake = types.SimpleNamespace(_space=None, _gp=None, _random_state=None)      # no engine: every error comes before the gate
    with pytest.raises(ValueError, match=match):
        suggest_local(fake, **kw)
    with pytest.raises(NotImplementedError, match="not on the engine"):
        suggest_local(fake)


def test_suggest_local_gates_without_a_host_fallback():
    fake = type("Fake", (FakeEngine,), {"nn_acq_argbest": None})      # the gate only asks whether the engine has the call
    B.check_shared_refusals(suggest_local, lambda **kw: B.suggest_driver(fake, **kw), "suggest_local")
    assert issubclass(ConstrainedSpaceNotImplemented, NotImplementedError)      # what a constrained space is refused with
