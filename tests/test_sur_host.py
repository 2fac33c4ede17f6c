"""CPU: sur_truth's G against mpmath's integral and, at r2 = 1, against Phi(h) Phi(-h); the reference's own fp64-versus-longdouble
spread on every case of tests/test_gpu_sur.py; include/gpls.h: C99 on its own, both libraries export exactly its names, _lib binds
them."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy import special

import sur_truth as T
import test_gpu_sur as GPU
from bayesianoptimization_amd import _lib
from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")


@pytest.mark.parametrize("h", [0.0, 0.3, 1.2, 2.0, 4.0, 8.0])
def test_G_against_mpmath(h):
    import mpmath as mp

    for r2 in (1e-6, 0.2, 0.5, 0.9, 0.999, 1.0):
        want = float(mp.quad(lambda th: mp.exp(-h * h / (1 + mp.sin(th))), [0, mp.asin(r2)]) / (2 * mp.pi))
        assert abs(float(T.G(h * h, r2)) - want) <= 1e-16 + 1e-14 * want, (h, r2)
    assert abs(float(T.G(h * h, 1.0)) - special.ndtr(h) * special.ndtr(-h)) <= 1e-16 + 4e-16 * special.ndtr(-h)
    assert float(T.G(h * h, 0.0)) == 0.0


@pytest.mark.parametrize("case", GPU.CASES, ids=lambda c: "J{}-N{}-M{}-d{}-k{}".format(*c[:5]))
def test_the_truths_own_spread(case):
    X, yn, ls, Xc, pts, om, c, w, level, alpha = GPU.inputs(*case)
    omega = np.full(case[0], 1.0 / case[0]) if om is None else om
    both = [T.sur(case[4], X, yn, ls, alpha, Xc[:65], pts, omega, level, GPU.Y_MEAN, GPU.Y_STD, c, w, dtype=t)
            for t in (np.longdouble, np.float64)]
    spread = max(np.abs(both[0][0] - both[1][0]).max(), np.abs(both[0][1] - both[1][1]).max(), abs(both[0][2] - both[1][2]))
    print(f"{case}: spread {spread:.2e}")
    assert spread <= 2.5e-10 and alpha >= 1e-4


def test_the_header_is_c99_and_both_libraries_export_exactly_its_names(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no host C compiler")
    (tmp_path / "only.c").write_text('#include "gpls.h"\nint main(void) { return GPLS_MAX_POINTS == 4096 ? 0 : 1; }\n')
    for flags in ([], ["-DGPBO_DEBUG"]):
        subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", *flags, "-I", INCLUDE,
                        str(tmp_path / "only.c")], check=True)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "gpls.h")).read(), flags=re.S)
    head, rest = src.split("#ifdef GPBO_DEBUG", 1)
    product, debug = (sorted(set(re.findall(r"\b(gpls_\w+)\s*\(", part))) for part in (head, rest.split("#endif", 1)[0]))
    assert product == ["gpls_sur_argbest"] == sorted(_lib.LS_SIGNATURES) and debug == ["gpls_debug_stage_ms"] == sorted(_lib.LS_DEBUG_SIGNATURES)
    assert _lib.MAX_LS_POINTS == 4096
    for path, names in ((_lib.LIB_PATH, product), (_lib.DEBUG_LIB_PATH, sorted(product + debug))):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert sorted({ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("gpls")}) == names, path
    for name, table in (("gpls_sur_argbest", _lib.LS_SIGNATURES), ("gpls_debug_stage_ms", _lib.LS_DEBUG_SIGNATURES)):
        args = re.search(name + r"\s*\((.*?)\);", src, flags=re.S).group(1)
        assert len(args.split(",")) == len(table[name][1]), name
