"""CPU: how gpmo_cnhvi_greedy lays out its workspace (bayesianoptimization_amd/csrc/cmo_plan.h), compiled for the host with the
system C++ compiler as its siblings are, and checked over (T, S) x M x B x (d, DP) x q x with and without the two stages:

  * no two regions overlap: each region's extent, worked out here from the sizes of the arrays themselves, ends at or before the
    next region's start, and the last ends at `doubles`;
  * every region starts at an even offset (the blocks, the fronts and the scaled base points are read 16 bytes at a time);
  * a stage is present only when asked for, the mask is M BYTES, and the sizes include/gpmo.h states for the workspace are the ones
    the plan gives (the whole buffer is their sum up to the rounding of each region to 16 bytes);
  * rows written out by hand, so that a constant of the header moved by one step changes at least one of them."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "bayesianoptimization_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
L = 128      # GPBO_MAX_QNEHVI_FRONT

SHIM = r"""
#include "cmo_plan.h"
using namespace gpbo;
extern "C" void block(int T, int S, long long M, int B, int d, int DP, int q, int values, int base_values, long long* o) {
  const CmoBlock b = cmo_block(T, S, M, B, d, DP, q, values != 0, base_values != 0);
  const int64_t v[] = {b.vals, b.basev, b.front, b.front0, b.size, b.size0, b.viol, b.violb, b.stage, b.stageb, b.base, b.base_s,
                       b.rec, b.flag, b.mask, b.ldb, b.doubles};
  for (int i = 0; i < 17; ++i) o[i] = v[i];
}
"""

FIELDS = ["vals", "basev", "front", "front0", "size", "size0", "viol", "violb", "stage", "stageb", "base", "base_s", "rec", "flag",
          "mask", "ldb", "doubles"]
GRID = list(itertools.product(((1, 1), (10, 5), (256, 16)), (1, 5, 63, 64, (1 << 17) + 3, 1 << 20), (0, 1, 66, 16384),
                              ((1, 4), (5, 8), (17, 32)), (1, 8, 63, 64), (0, 1), (0, 1)))


@pytest.fixture(scope="module")
def block(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("cmo_plan"))
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src, so = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "libcmoplan.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-fPIC", "-shared", "-I" + CSRC, "-I" + INCLUDE, src, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.block.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong] + [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_longlong)]

    def call(T, S, M, B, d, DP, q, values, base_values):
        out = (ctypes.c_longlong * len(FIELDS))()
        lib.block(T, S, M, B, d, DP, q, values, base_values, out)
        return dict(zip(FIELDS, out))
    return call


def extents(T, S, M, B, d, DP, q, values, base_values):
    """doubles each region needs, from the arrays themselves (ints two to a double, mask bytes eight to a double)"""
    return {"vals": 2 * T * M, "basev": 2 * T * B, "front": T * L * 2, "front0": T * L * 2, "size": (T + 1) // 2,
            "size0": (T + 1) // 2, "viol": S * M, "violb": S * B, "stage": S * M if values else 0, "stageb": S * B if base_values else 0,
            "base": B * d, "base_s": B * DP, "rec": 3 * q, "flag": 1, "mask": (M + 7) // 8}


def test_no_two_regions_overlap_and_every_region_is_aligned(block):
    regions = FIELDS[:15]
    for (T, S), M, B, (d, DP), q, values, base_values in GRID:
        args = (T, S, M, B, d, DP, q, values, base_values)
        b, need = block(*args), extents(*args)
        assert b["vals"] == 0 and b["ldb"] == B
        for name, nxt in zip(regions, regions[1:] + ["doubles"]):
            assert b[name] % 2 == 0, (args, name)
            assert b[name] + need[name] <= b[nxt], (args, name, "runs into", nxt)
            assert b[nxt] - (b[name] + need[name]) <= 1 or name == "flag", (args, name, "leaves a gap")
        assert b["mask"] - b["flag"] == 2
        assert b["stage"] == b["stageb"] if not values else b["stageb"] - b["stage"] >= S * M
        assert b["base"] == b["stageb"] if not base_values else b["base"] - b["stageb"] >= S * B


def test_the_sizes_the_header_states(block):
    """include/gpmo.h: the block 16 T M bytes, one group's violations 8 S M (+ 8 S M for the stage), at the base points
    8 (2 T + S) n_base (+ 8 S n_base), the fronts 4096 T, their sizes 8 T (rounded up to 16), the base points 8 n_base (d + DP), the
    records 24 q, the flag 16 and the mask M bytes (rounded up to 8)"""
    with open(os.path.join(INCLUDE, "gpmo.h")) as f:
        text = " ".join(f.read().split())
    for words in ("the block 16 T M bytes", "one group's violations * 8 S M (+ 8 S M for the stage with values_out)",
                  "8 (2 T + S) n_base (+ 8 S n_base with base_values_out)", "fronts 4096 T", "their sizes 8 T",
                  "8 n_base (d + DP)", "the records 24 q", "the flag 16", "the mask M bytes"):
        assert words.replace(" * ", " ") in text.replace(" * ", " "), words
    for (T, S), M, B, (d, DP), q, values, base_values in GRID:
        b = block(T, S, M, B, d, DP, q, values, base_values)
        stated = (16 * T * M + 8 * S * M * (1 + values) + 8 * (2 * T + S) * B + 8 * S * B * base_values + 4096 * T
                  + 2 * ((4 * T + 7) // 8 * 8) + 8 * B * (d + DP) + 24 * q + 16 + (M + 7) // 8 * 8)
        assert 0 <= 8 * b["doubles"] - stated <= 8 * 13, "at most one double of rounding per region"


# (T, S, M, B, d, DP, q, values, base_values) -> FIELDS, worked out by hand from the layout in the header's comment
ROWS = {
    # everything 1, no base point, no stage: vals 2 | fronts 256 + 256 | sizes 1 -> 2 each | viol 1 -> 2 | rec 3 -> 4 | flag 2 | mask 1
    (1, 1, 1, 0, 1, 4, 1, 0, 0): (0, 2, 2, 258, 514, 516, 518, 520, 520, 520, 520, 520, 520, 524, 526, 0, 527),
    # ... one base point and both stages: basev 2, violb 1 -> 2, stage 1 -> 2, stageb 1 -> 2, base 1 -> 2, base_s 4
    (1, 1, 1, 1, 1, 4, 1, 1, 1): (0, 2, 4, 260, 516, 518, 520, 522, 524, 526, 528, 530, 534, 538, 540, 1, 541),
    # T = 10, S = 5, M = 63, B = 66, d = 2, DP = 4, q = 8: vals 1260 | basev 1320 | fronts 2560 each | sizes 5 -> 6 each | viol 315 -> 316
    # | violb 330 | base 132 | base_s 264 | rec 24 | flag 2 | mask 8
    (10, 5, 63, 66, 2, 4, 8, 0, 0): (0, 1260, 2580, 5140, 7700, 7706, 7712, 8028, 8358, 8358, 8358, 8490, 8754, 8778, 8780, 66, 8788),
    # ... with the candidates' stage (315 -> 316) | q = 63: 189 -> 190
    (10, 5, 63, 66, 2, 4, 63, 1, 0): (0, 1260, 2580, 5140, 7700, 7706, 7712, 8028, 8358, 8674, 8674, 8806, 9070, 9260, 9262, 66, 9270),
}


@pytest.mark.parametrize("args", sorted(ROWS))
def test_rows_worked_out_by_hand(block, args):
    got = block(*args)
    assert tuple(got[f] for f in FIELDS) == ROWS[args]
