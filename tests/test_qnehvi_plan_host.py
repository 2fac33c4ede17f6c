"""CPU: how gpbo_qnhvi_greedy lays out its workspace and stages its fronts (bayesianoptimization_amd/csrc/qnehvi_plan.h), compiled
for the host with the system C++ compiler and checked

  * against the sizes of the arrays themselves over T in {1, 3, 10, 256} x M in {1, 5, 63, 64, 2^17 + 3, 2^20} x B in {0, 1, 66,
    16384} x (d, DP) in {(1, 4), (5, 8), (17, 32)} x q in {1, 8, 64}: the regions in order, every one at an even offset (the blocks
    and the fronts are read 16 bytes at a time), no two overlapping, the sizes T INTS, the mask M BYTES long, the block 16 T M bytes —
    4 GiB at T = 256, M = 2^20, as include/gpbo.h states;
  * against rows written out below;
  * on both sides of every edge of its rules: the LDS stage of 16 draws (T = 15 | 16 | 17: one chunk, one full chunk, a second
    one), its bytes against the 160 KiB of a CU, and the score kernel's thread rule, which is qnei_plan.h's (M odd | even).
A constant of the header moved by one step changes at least one row."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "bayesianoptimization_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")

SHIM = r"""
#include "qnehvi_plan.h"
using namespace gpbo;
extern "C" {
void block(int T, long long M, int B, int d, int DP, int q, long long* o) {
  const QnehviBlock b = qnehvi_block(T, M, B, d, DP, q);
  const int64_t v[] = {b.vals, b.basev, b.front, b.front0, b.size, b.size0, b.base, b.base_s, b.rec, b.flag, b.mask, b.ldb, b.doubles};
  for (int i = 0; i < 13; ++i) o[i] = v[i];
}
int chunk_draws(int T) { return qnehvi_chunk_draws(T); }
int chunks(int T) { return qnehvi_chunks(T); }
long long lds_bytes() { return QNEHVI_LDS_BYTES; }
int front() { return QNEHVI_FRONT; }
int strips() { return QNEHVI_STRIPS; }
int chunk() { return QNEHVI_CHUNK; }
int items(long long M) { return qnei_items(M); }
long long blocks(long long M) { return qnei_score_blocks(M); }
int block_threads() { return QNEI_BLOCK; }
int max_draws() { return QNEI_MAX_DRAWS; }
}
"""

FIELDS = ["vals", "basev", "front", "front0", "size", "size0", "base", "base_s", "rec", "flag", "mask", "ldb", "doubles"]
GRID = list(itertools.product((1, 3, 10, 256), (1, 5, 63, 64, (1 << 17) + 3, 1 << 20), (0, 1, 66, 16384),
                              ((1, 4), (5, 8), (17, 32)), (1, 8, 64)))


class Plan:
    def __init__(self, tmp_dir, header_dir=CSRC):
        cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
        if cxx is None:
            pytest.fail("no host C++ compiler")
        src, so = os.path.join(tmp_dir, "shim.cpp"), os.path.join(tmp_dir, "libqnehviplan.so")
        with open(src, "w") as f:
            f.write(SHIM)
        subprocess.run([cxx, "-std=c++17", "-O1", "-fPIC", "-shared", "-I" + header_dir, "-I" + CSRC, "-I" + INCLUDE, src, "-o", so],
                       check=True)
        L = self.L = ctypes.CDLL(so)
        L.block.argtypes = [ctypes.c_int, ctypes.c_longlong] + [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_longlong)]
        L.lds_bytes.restype = ctypes.c_longlong
        L.items.argtypes = [ctypes.c_longlong]
        L.blocks.argtypes = [ctypes.c_longlong]
        L.blocks.restype = ctypes.c_longlong

    def block(self, T, M, B, d, DP, q):
        out = (ctypes.c_longlong * len(FIELDS))()
        self.L.block(T, M, B, d, DP, q, out)
        return tuple(out)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return Plan(str(tmp_path_factory.mktemp("qnehvi_plan")))


# (T, M, B, d, DP, q) -> FIELDS, worked out by hand from the layout in the header's comment
BLOCK_ROWS = {
    (1, 1, 0, 1, 4, 1): (0, 2, 2, 258, 514, 516, 518, 518, 518, 520, 522, 0, 523),
    (3, 5, 1, 1, 4, 2): (0, 30, 36, 804, 1572, 1574, 1576, 1578, 1586, 1590, 1592, 1, 1593),
    (10, 63, 66, 2, 4, 8): (0, 1260, 2580, 5140, 7700, 7706, 7712, 7844, 8372, 8388, 8390, 66, 8398),
    (256, 1 << 20, 4096, 16, 16, 64): (0, 536870912, 538968064, 539033600, 539099136, 539099264, 539099392, 539164928, 539296000,
                                       539296128, 539296130, 4096, 539427202),
}
CHUNK_ROWS = {1: (1, 1), 10: (10, 1), 15: (15, 1), 16: (16, 1), 17: (16, 2), 32: (16, 2), 33: (16, 3), 256: (16, 16)}


def mismatches(plan):
    L = plan.L
    bad = []
    bad += [("block", k) for k, v in BLOCK_ROWS.items() if plan.block(*k) != v]
    bad += [("chunk", T) for T, v in CHUNK_ROWS.items() if (L.chunk_draws(T), L.chunks(T)) != v]
    bad += [("lds",)] if L.lds_bytes() != 16 * 129 * 16 + 64 else []
    bad += [("front",)] if (L.front(), L.strips(), L.chunk()) != (128, 129, 16) else []
    bad += [("threads",)] if L.block_threads() != 256 or L.max_draws() != 256 else []
    return bad


def test_the_tables(plan):
    assert mismatches(plan) == []


def test_the_block_over_the_whole_grid(plan):
    for T, M, B, (d, DP), q in GRID:
        b = dict(zip(FIELDS, plan.block(T, M, B, d, DP, q)))
        assert b["ldb"] == B
        sizes = [("vals", 16 * T * M), ("basev", 16 * T * B), ("front", 16 * 128 * T), ("front0", 16 * 128 * T), ("size", 4 * T),
                 ("size0", 4 * T), ("base", 8 * B * d), ("base_s", 16 * B * DP), ("rec", 16 * q), ("flag", 4), ("mask", M)]
        at = 0
        for name, n in sizes:
            start = 8 * b[name]
            assert at <= start < at + 16 and b[name] % 2 == 0, (name, T, M, B, d, q)      # behind the one before, even, no hole beyond the rounding
            at = start + n
        assert at <= 8 * b["doubles"] < at + 8
    # the figure the header states, and objective 1's block starts on a 16-byte boundary whenever pairs are read
    b = dict(zip(FIELDS, plan.block(256, 1 << 20, 4096, 16, 16, 64)))
    assert 8 * (b["basev"] - b["vals"]) == 4 << 30
    for T, M in itertools.product((1, 3, 255), (2, 64, 1 << 20)):
        assert plan.L.items(M) == 2 and (T * M) % 2 == 0


def test_the_rules_on_both_sides_of_their_edges(plan):
    L = plan.L
    # the LDS stage: T <= 16 stages once, 17 needs a second chunk; every draw is in exactly one chunk
    assert [(L.chunk_draws(T), L.chunks(T)) for T in (15, 16, 17)] == [(15, 1), (16, 1), (16, 2)]
    for T in range(1, 257):
        n, c = L.chunks(T), L.chunk()
        assert (n - 1) * c < T <= n * c and L.chunk_draws(T) == min(T, c)
    # four workgroups' stages fit a CU's 160 KiB, and a stage holds the largest front's strips for every draw of a chunk
    assert 4 * L.lds_bytes() <= 160 * 1024 < 5 * L.lds_bytes()
    assert L.lds_bytes() == L.chunk() * (L.strips() * 16 + 4) and L.strips() == L.front() + 1
    # the thread rule is qnei_plan.h's
    assert [L.items(M) for M in (62, 63, 64, 65)] == [2, 1, 2, 1]
    assert [L.blocks(M) for M in (256, 257, 512, 514)] == [1, 2, 1, 2]


MOVED = [
    ("QNEHVI_CHUNK = 16", "QNEHVI_CHUNK = 15"), ("QNEHVI_FRONT + 1", "QNEHVI_FRONT + 2"), ("T < QNEHVI_CHUNK ? T", "T < QNEHVI_CHUNK - 1 ? T"),
    ("(T + QNEHVI_CHUNK - 1) / QNEHVI_CHUNK", "(T + QNEHVI_CHUNK) / QNEHVI_CHUNK"), ("QNEHVI_STRIPS * 16 +", "QNEHVI_STRIPS * 8 +"),
    ("b.ldb = B", "b.ldb = B + 1"), ("b.vals + 2 * T * M", "b.vals + 2 * T * M + 2"), ("b.basev + 2 * T * b.ldb", "b.basev + 2 * T * b.ldb + 2"),
    ("b.front0 = b.front + T * L * 2", "b.front0 = b.front + T * L * 2 + 2"), ("b.size = b.front0 + T * L * 2", "b.size = b.front0 + T * L * 2 + 2"),
    ("b.size + (T + 1) / 2", "b.size + (T + 1) / 2 + 2"), ("b.size0 + (T + 1) / 2", "b.size0 + (T + 1) / 2 + 2"),
    ("b.base + B * d", "b.base + B * d + 2"), ("b.base_s + 2 * B * DP", "b.base_s + 2 * B * DP + 2"), ("b.rec + 2 * q", "b.rec + 2 * q + 2"),
    ("b.mask = b.flag + 2", "b.mask = b.flag + 4"), ("(M + 7) / 8", "(M + 8) / 8"),
]


@pytest.mark.parametrize("old,new", MOVED, ids=["chunk", "strips", "chunk_draws", "chunks", "lds", "ldb", "basev", "front", "front0", "size",
                                                "size0", "base", "base_s", "rec", "flag", "mask", "doubles"])
def test_a_moved_constant_changes_a_row(tmp_path, old, new):
    src = open(os.path.join(CSRC, "qnehvi_plan.h")).read()
    assert src.count(old) == 1, old
    with open(tmp_path / "qnehvi_plan.h", "w") as f:
        f.write(src.replace(old, new))
    assert mismatches(Plan(str(tmp_path), header_dir=str(tmp_path))) != []
