"""CPU: the workspace and the dispatch of gpbo_sample_paths_constrained (bayesianoptimization_amd/csrc/path_plan.h: constrained_block,
path_epilogue), compiled for the host with the system C++ compiler: the regions in order, back to back up to the padding that keeps
every one of them on an even offset (the kernel reads points as double2), no room for values unless they are asked for, room for
16 fallback points of DP coordinates and for all S paths at each; the constraints fold in slot order and the objective selects."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "bayesianoptimization_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
MAX_PATHS = 16

SHIM = r"""
#include "path_plan.h"
using namespace gpbo;
extern "C" {
void cblock(int S, long long M, int DP, int values, long long* o) {
  const ConstrainedBlock b = constrained_block(S, M, DP, values != 0);
  const int64_t v[] = {b.viol, b.vals, b.pts, b.f, b.doubles};
  for (int i = 0; i < 5; ++i) o[i] = v[i];
}
int epilogue(int slot) { return path_epilogue(slot); }
int plain() { return PATH_PLAIN; }
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    tmp = str(tmp_path_factory.mktemp("constrained_plan"))
    src, so = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "libcplan.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-fPIC", "-shared", "-I" + CSRC, "-I" + INCLUDE, src, "-o", so], check=True)
    L = ctypes.CDLL(so)
    L.cblock.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)]
    return L


def block(plan, S, M, DP, values):
    out = (ctypes.c_longlong * 5)()
    plan.cblock(S, M, DP, int(values), out)
    return tuple(out)


def test_written_out_rows(plan):
    assert block(plan, 1, 1, 4, False) == (0, 2, 2, 66, 82)
    assert block(plan, 1, 1, 4, True) == (0, 2, 4, 68, 84)
    assert block(plan, 5, 257, 8, True) == (0, 1286, 2572, 2700, 2780)
    assert block(plan, 16, (1 << 30) + 1, 64, False) == (0, 16 * ((1 << 30) + 1), 16 * ((1 << 30) + 1), 16 * ((1 << 30) + 1) + 1024,
                                                         16 * ((1 << 30) + 1) + 1024 + 256)


@pytest.mark.parametrize("values", [False, True])
def test_regions_in_order_even_and_large_enough(plan, values):
    for S, M, DP in itertools.product((1, 3, 4, 5, 16), (1, 2, 63, 257, (1 << 17) + 3), (4, 8, 16, 32, 64)):
        viol, vals, pts, f, doubles = block(plan, S, M, DP, values)
        assert viol == 0 and all(o % 2 == 0 for o in (vals, pts, f))
        assert S * M <= vals - viol <= S * M + 1                       # viol [S][M], padded to an even size
        assert pts - vals == ((vals - viol) if values else 0)          # one slot's values, only when asked for
        assert f - pts == MAX_PATHS * DP and doubles - f == S * MAX_PATHS


def test_the_constraints_fold_in_slot_order_and_the_objective_selects(plan):
    write, add, key = plan.epilogue(1), plan.epilogue(2), plan.epilogue(0)
    assert len({plan.plain(), write, add, key}) == 4 and plan.plain() == 0
    assert [plan.epilogue(j) for j in range(2, 8)] == [add] * 6
