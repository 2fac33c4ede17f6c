"""CPU: how gpbo_cnei_greedy lays out its workspace (bayesianoptimization_amd/csrc/cnei_plan.h), compiled for the host with the
system C++ compiler and checked

  * against the sizes of the arrays themselves over (T, S) in {(1, 1), (10, 5), (256, 16)} x M in {1, 5, 63, 64, 2^17 + 3, 2^20} x
    B in {0, 1, 66, 16384} x (d, DP) in {(1, 4), (5, 8), (17, 32)} x q in {1, 8, 63, 64} x with and without the two stages: the
    regions in order, back to back up to the rounding, every one at an even offset (the block and the scaled base points are read 16
    bytes at a time), no two overlapping, the mask M BYTES long, a stage present only when asked for;
  * against rows written out below, on both sides of every edge: B = 0 | 1, an odd | even product before each region, q odd | even
    (a record is three doubles), M a multiple of 8 | one more, each stage on | off.
A constant of the header moved by one step changes at least one row."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "bayesianoptimization_amd", "csrc")

SHIM = r"""
#include "cnei_plan.h"
using namespace gpbo;
extern "C" void block(int T, int S, long long M, int B, int d, int DP, int q, int values, int base_values, long long* o) {
  const CneiBlock b = cnei_block(T, S, M, B, d, DP, q, values != 0, base_values != 0);
  const int64_t v[] = {b.vals, b.base, b.m, b.m0, b.viol, b.violb, b.stage, b.stageb, b.pts, b.pts_s, b.rec, b.mask, b.ldb, b.doubles};
  for (int i = 0; i < 14; ++i) o[i] = v[i];
}
"""

FIELDS = ["vals", "base", "m", "m0", "viol", "violb", "stage", "stageb", "pts", "pts_s", "rec", "mask", "ldb", "doubles"]
GRID = list(itertools.product(((1, 1), (10, 5), (256, 16)), (1, 5, 63, 64, (1 << 17) + 3, 1 << 20), (0, 1, 66, 16384),
                              ((1, 4), (5, 8), (17, 32)), (1, 8, 63, 64), (0, 1), (0, 1)))


class Plan:
    def __init__(self, tmp_dir, header_dir=CSRC):
        cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
        if cxx is None:
            pytest.fail("no host C++ compiler")
        src, so = os.path.join(tmp_dir, "shim.cpp"), os.path.join(tmp_dir, "libcneiplan.so")
        with open(src, "w") as f:
            f.write(SHIM)
        subprocess.run([cxx, "-std=c++17", "-O1", "-fPIC", "-shared", "-I" + header_dir, src, "-o", so], check=True)
        self.L = ctypes.CDLL(so)
        self.L.block.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong] + [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_longlong)]

    def block(self, T, S, M, B, d, DP, q, values, base_values):
        out = (ctypes.c_longlong * len(FIELDS))()
        self.L.block(T, S, M, B, d, DP, q, values, base_values, out)
        return tuple(out)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return Plan(str(tmp_path_factory.mktemp("cnei_plan")))


# (T, S, M, B, d, DP, q, values, base_values) -> FIELDS, worked out by hand from the layout in the header's comment
BLOCK_ROWS = {
    # everything 1, no base point, no stage: each region rounded up to the next even offset; rec 3 -> 4; one mask double
    (1, 1, 1, 0, 1, 4, 1, 0, 0): (0, 2, 2, 4, 6, 8, 8, 8, 8, 8, 8, 12, 0, 13),
    # ... one base point and both stages
    (1, 1, 1, 1, 1, 4, 1, 1, 1): (0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 22, 26, 1, 27),
    # T = 10, S = 5, M = 63, B = 66, d = 2, DP = 4, q = 8: vals 630 | base 660 | m 10 | m0 10 | viol 315 -> 316 | violb 330 |
    # no stage | pts 132 | pts_s 264 | rec 24 | mask 8 doubles
    (10, 5, 63, 66, 2, 4, 8, 0, 0): (0, 630, 1290, 1300, 1310, 1626, 1956, 1956, 1956, 2088, 2352, 2376, 66, 2384),
    # ... with the candidates' stage (315 -> 316) | with the base points' (330)
    (10, 5, 63, 66, 2, 4, 8, 1, 0): (0, 630, 1290, 1300, 1310, 1626, 1956, 2272, 2272, 2404, 2668, 2692, 66, 2700),
    (10, 5, 63, 66, 2, 4, 8, 0, 1): (0, 630, 1290, 1300, 1310, 1626, 1956, 1956, 2286, 2418, 2682, 2706, 66, 2714),
    # q = 63: 189 doubles of records -> 190; M = 64: exactly 8 mask doubles
    (10, 5, 64, 66, 2, 4, 63, 0, 0): (0, 640, 1300, 1310, 1320, 1640, 1970, 1970, 1970, 2102, 2366, 2556, 66, 2564),
    # the workload: T = 256, S = 16, M = 2^20, B = 4096 + 8, d = 16, DP = 16, q = 8
    (256, 16, 1 << 20, 4104, 16, 16, 8, 0, 0): (0, 268435456, 269486080, 269486336, 269486592, 286263808, 286329472, 286329472,
                                                 286329472, 286395136, 286460800, 286460824, 4104, 286591896),
}


def mismatches(plan):
    return [k for k, v in BLOCK_ROWS.items() if plan.block(*k) != v]


def test_the_tables(plan):
    assert mismatches(plan) == []


def test_the_block_over_the_whole_grid(plan):
    for (T, S), M, B, (d, DP), q, values, base_values in GRID:
        b = dict(zip(FIELDS, plan.block(T, S, M, B, d, DP, q, values, base_values)))
        assert b["ldb"] == B
        sizes = [("vals", 8 * T * M), ("base", 8 * T * B), ("m", 8 * T), ("m0", 8 * T), ("viol", 8 * S * M), ("violb", 8 * S * B),
                 ("stage", 8 * S * M * values), ("stageb", 8 * S * B * base_values), ("pts", 8 * B * d), ("pts_s", 8 * B * DP),
                 ("rec", 24 * q), ("mask", M)]
        at = 0
        for name, n in sizes:
            start = 8 * b[name]
            # behind the one before, even, no hole beyond the rounding
            assert at <= start < at + 16 and b[name] % 2 == 0, (name, T, S, M, B, d, q, values, base_values)
            at = start + n
        assert at <= 8 * b["doubles"] < at + 8
    # the block is 8 T M bytes: 2 GiB at T = 256, M = 2^20
    b = dict(zip(FIELDS, plan.block(256, 16, 1 << 20, 4096, 16, 16, 64, 0, 0)))
    assert 8 * (b["base"] - b["vals"]) == 2 << 30


MOVED = [
    ("(x + 1) / 2 * 2", "(x + 2) / 2 * 2"), ("b.ldb = B", "b.ldb = B + 1"), ("b.vals + T * M", "b.vals + T * M + 2"),
    ("b.base + T * B", "b.base + T * B + 2"), ("b.m + T)", "b.m + T + 2)"), ("b.m0 + T)", "b.m0 + T + 2)"),
    ("b.viol + S * M", "b.viol + S * M + 2"), ("b.violb + S * B", "b.violb + S * B + 2"), ("(values ? S * M : 0)", "(values ? S * M : 2)"),
    ("(base_values ? S * B : 0)", "(base_values ? S * B : 2)"), ("b.pts + B * d", "b.pts + B * d + 2"),
    ("b.pts_s + B * DP", "b.pts_s + B * DP + 2"), ("b.rec + 3 * q", "b.rec + 2 * q"), ("(M + 7) / 8", "(M + 8) / 8"),
]


@pytest.mark.parametrize("old,new", MOVED, ids=["even", "ldb", "base", "m", "m0", "viol", "violb", "stage", "stageb", "pts", "pts_s",
                                                "rec", "mask", "doubles"])
def test_a_moved_constant_changes_a_row(tmp_path, old, new):
    src = open(os.path.join(CSRC, "cnei_plan.h")).read()
    assert src.count(old) == 1, old
    with open(tmp_path / "cnei_plan.h", "w") as f:
        f.write(src.replace(old, new))
    assert mismatches(Plan(str(tmp_path), header_dir=str(tmp_path))) != []
