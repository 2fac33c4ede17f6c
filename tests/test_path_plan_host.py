"""CPU: how the posterior function draws' workspace is laid out and their kernels dispatched (bayesianoptimization_amd/csrc/
path_plan.h), compiled for the host with the system C++ compiler and checked against the tables written out below and against the
sizes of the arrays themselves:

  * path_block over S in {1, 4, 5, 16} x F in {1, 64, 65, 4096} x (N, NP) in {(1, 64), (64, 64), (65, 128), (700, 704)} x d in
    {1, 4, 5, 64} x n_runs in {0, 1, 7, 128} (7 is odd: status and evals start on a half double): the regions in order and back to
    back up to the stated slack (R ints behind status, R ints behind evals), start_idx on 8 bytes, status and evals inside the block
    and apart, the ascent part the 2 d + 3 R d + 4 R doubles its caller used to ask for, nothing behind V when n_runs = 0;
  * which instance of path_eval_kernel serves S paths on both sides of S = 1 | 2 and 4 | 5, its workgroup size on both sides of
    M = 2^17 - 1 | 2^17, the features' scale, the default iteration limit.

The tables were printed once from a verbatim copy of the expressions as they stood in launch_path_weights (posterior_paths.hip:
the running pointers om_d ... V and the size handed to ensure), launch_path_ascent (path_ascent.hip: lo_d ... eval_d, casts included)
and path_ascent_doubles, before the header replaced them: offsets as differences of the pointers from the workspace's start, in
doubles (status / evals: in ints).  All 1 024 cases of the grid above x 17 values were compared with the header then, no difference;
BLOCK_ROWS keeps the S x F plane, the (N, NP) line and the d x n_runs plane through (5, 65, 65, 128, 5, 7).  The old code had no
ascent part for n_runs = 0: those rows give its (empty) arrays at the end of the block.  A constant of the header moved by one step
changes at least one row (test_a_moved_constant_changes_a_row moves each)."""
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
#include "path_plan.h"
using namespace gpbo;
extern "C" {
void block(int S, int F, int N, int NP, int d, int n_runs, long long* o) {
  const PathBlock b = path_block(S, F, N, NP, d, n_runs);
  const int64_t v[] = {b.omega, b.phase, b.weights, b.eps, b.G, b.T, b.V, b.lo, b.hi, b.starts, b.x, b.g, b.f, b.start_idx, b.status,
                       b.evals, b.doubles};
  for (int i = 0; i < 17; ++i) o[i] = v[i];
}
int ns(int S) { return path_eval_ns(S); }
unsigned threads(long long M) { return path_eval_threads(M); }
double scale(double amplitude, int F) { return path_feature_scale(amplitude, F); }
int default_max_iter() { return PATH_DEFAULT_MAX_ITER; }
}
"""

FIELDS = ["omega", "phase", "weights", "eps", "G", "T", "V", "lo", "hi", "starts", "x", "g", "f", "start_idx", "status", "evals",
          "doubles"]
GRID = list(itertools.product((1, 4, 5, 16), (1, 64, 65, 4096), ((1, 64), (64, 64), (65, 128), (700, 704)), (1, 4, 5, 64),
                              (0, 1, 7, 128)))


class Plan:
    def __init__(self, tmp_dir, header_dir=CSRC):
        cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
        if cxx is None:
            pytest.fail("no host C++ compiler")
        src, so = os.path.join(tmp_dir, "shim.cpp"), os.path.join(tmp_dir, "libpathplan.so")
        with open(src, "w") as f:
            f.write(SHIM)
        subprocess.run([cxx, "-std=c++17", "-O1", "-fPIC", "-shared", "-I" + header_dir, "-I" + INCLUDE, src, "-o", so], check=True)
        L = self.L = ctypes.CDLL(so)
        L.threads.argtypes = [ctypes.c_longlong]
        L.threads.restype = ctypes.c_uint
        L.scale.argtypes = [ctypes.c_double, ctypes.c_int]
        L.scale.restype = ctypes.c_double

    def block(self, S, F, N, NP, d, n_runs):
        out = (ctypes.c_longlong * len(FIELDS))()
        self.L.block(S, F, N, NP, d, n_runs, out)
        return tuple(out)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return Plan(str(tmp_path_factory.mktemp("path_plan")))


# (S, F, N, NP, d, n_runs) -> FIELDS
BLOCK_ROWS = {
    (1, 1, 65, 128, 5, 7): (0, 5, 6, 7, 72, 200, 328, 456, 461, 466, 501, 536, 571, 578, 1170, 1184, 599),
    (1, 64, 65, 128, 5, 7): (0, 320, 384, 448, 513, 641, 769, 897, 902, 907, 942, 977, 1012, 1019, 2052, 2066, 1040),
    (1, 65, 65, 128, 5, 7): (0, 325, 390, 455, 520, 648, 776, 904, 909, 914, 949, 984, 1019, 1026, 2066, 2080, 1047),
    (1, 4096, 65, 128, 5, 7): (0, 20480, 24576, 28672, 28737, 28865, 28993, 29121, 29126, 29131, 29166, 29201, 29236, 29243, 58500,
                               58514, 29264),
    (4, 1, 65, 128, 5, 7): (0, 5, 6, 10, 270, 782, 1294, 1806, 1811, 1816, 1851, 1886, 1921, 1928, 3870, 3884, 1949),
    (4, 64, 65, 128, 5, 7): (0, 320, 384, 640, 900, 1412, 1924, 2436, 2441, 2446, 2481, 2516, 2551, 2558, 5130, 5144, 2579),
    (4, 65, 65, 128, 5, 7): (0, 325, 390, 650, 910, 1422, 1934, 2446, 2451, 2456, 2491, 2526, 2561, 2568, 5150, 5164, 2589),
    (4, 4096, 65, 128, 5, 7): (0, 20480, 24576, 40960, 41220, 41732, 42244, 42756, 42761, 42766, 42801, 42836, 42871, 42878, 85770,
                               85784, 42899),
    (5, 1, 65, 128, 5, 7): (0, 5, 6, 11, 336, 976, 1616, 2256, 2261, 2266, 2301, 2336, 2371, 2378, 4770, 4784, 2399),
    (5, 64, 65, 128, 5, 7): (0, 320, 384, 704, 1029, 1669, 2309, 2949, 2954, 2959, 2994, 3029, 3064, 3071, 6156, 6170, 3092),
    (5, 65, 65, 128, 5, 7): (0, 325, 390, 715, 1040, 1680, 2320, 2960, 2965, 2970, 3005, 3040, 3075, 3082, 6178, 6192, 3103),
    (5, 4096, 65, 128, 5, 7): (0, 20480, 24576, 45056, 45381, 46021, 46661, 47301, 47306, 47311, 47346, 47381, 47416, 47423, 94860,
                               94874, 47444),
    (16, 1, 65, 128, 5, 7): (0, 5, 6, 22, 1062, 3110, 5158, 7206, 7211, 7216, 7251, 7286, 7321, 7328, 14670, 14684, 7349),
    (16, 64, 65, 128, 5, 7): (0, 320, 384, 1408, 2448, 4496, 6544, 8592, 8597, 8602, 8637, 8672, 8707, 8714, 17442, 17456, 8735),
    (16, 65, 65, 128, 5, 7): (0, 325, 390, 1430, 2470, 4518, 6566, 8614, 8619, 8624, 8659, 8694, 8729, 8736, 17486, 17500, 8757),
    (16, 4096, 65, 128, 5, 7): (0, 20480, 24576, 90112, 91152, 93200, 95248, 97296, 97301, 97306, 97341, 97376, 97411, 97418, 194850,
                                194864, 97439),
    (5, 65, 1, 64, 5, 7): (0, 325, 390, 715, 720, 1040, 1360, 1680, 1685, 1690, 1725, 1760, 1795, 1802, 3618, 3632, 1823),
    (5, 65, 64, 64, 5, 7): (0, 325, 390, 715, 1035, 1355, 1675, 1995, 2000, 2005, 2040, 2075, 2110, 2117, 4248, 4262, 2138),
    (5, 65, 700, 704, 5, 7): (0, 325, 390, 715, 4215, 7735, 11255, 14775, 14780, 14785, 14820, 14855, 14890, 14897, 29808, 29822,
                              14918),
    (5, 65, 65, 128, 1, 0): (0, 65, 130, 455, 780, 1420, 2060, 2700, 2700, 2700, 2700, 2700, 2700, 2700, 5400, 5400, 2700),
    (5, 65, 65, 128, 1, 1): (0, 65, 130, 455, 780, 1420, 2060, 2700, 2701, 2702, 2703, 2704, 2705, 2706, 5414, 5416, 2709),
    (5, 65, 65, 128, 1, 7): (0, 65, 130, 455, 780, 1420, 2060, 2700, 2701, 2702, 2709, 2716, 2723, 2730, 5474, 5488, 2751),
    (5, 65, 65, 128, 1, 128): (0, 65, 130, 455, 780, 1420, 2060, 2700, 2701, 2702, 2830, 2958, 3086, 3214, 6684, 6940, 3598),
    (5, 65, 65, 128, 4, 0): (0, 260, 325, 650, 975, 1615, 2255, 2895, 2895, 2895, 2895, 2895, 2895, 2895, 5790, 5790, 2895),
    (5, 65, 65, 128, 4, 1): (0, 260, 325, 650, 975, 1615, 2255, 2895, 2899, 2903, 2907, 2911, 2915, 2916, 5834, 5836, 2919),
    (5, 65, 65, 128, 4, 7): (0, 260, 325, 650, 975, 1615, 2255, 2895, 2899, 2903, 2931, 2959, 2987, 2994, 6002, 6016, 3015),
    (5, 65, 65, 128, 4, 128): (0, 260, 325, 650, 975, 1615, 2255, 2895, 2899, 2903, 3415, 3927, 4439, 4567, 9390, 9646, 4951),
    (5, 65, 65, 128, 5, 0): (0, 325, 390, 715, 1040, 1680, 2320, 2960, 2960, 2960, 2960, 2960, 2960, 2960, 5920, 5920, 2960),
    (5, 65, 65, 128, 5, 1): (0, 325, 390, 715, 1040, 1680, 2320, 2960, 2965, 2970, 2975, 2980, 2985, 2986, 5974, 5976, 2989),
    (5, 65, 65, 128, 5, 128): (0, 325, 390, 715, 1040, 1680, 2320, 2960, 2965, 2970, 3610, 4250, 4890, 5018, 10292, 10548, 5402),
    (5, 65, 65, 128, 64, 0): (0, 4160, 4225, 4550, 4875, 5515, 6155, 6795, 6795, 6795, 6795, 6795, 6795, 6795, 13590, 13590, 6795),
    (5, 65, 65, 128, 64, 1): (0, 4160, 4225, 4550, 4875, 5515, 6155, 6795, 6859, 6923, 6987, 7051, 7115, 7116, 14234, 14236, 7119),
    (5, 65, 65, 128, 64, 7): (0, 4160, 4225, 4550, 4875, 5515, 6155, 6795, 6859, 6923, 7371, 7819, 8267, 8274, 16562, 16576, 8295),
    (5, 65, 65, 128, 64, 128): (0, 4160, 4225, 4550, 4875, 5515, 6155, 6795, 6859, 6923, 15115, 23307, 31499, 31627, 63510, 63766,
                                32011),
}
NS_ROWS = {1: 1, 2: 4, 3: 4, 4: 4, 5: 16, 8: 16, 16: 16}                      # S -> the NS instance of path_eval_kernel
THREAD_ROWS = {1: 64, 300: 64, 131071: 64, 131072: 256, 1048576: 256}        # M -> threads of a workgroup
SCALE_ROWS = {      # (amplitude, F) -> fs = sqrt(2 amplitude / F)
    (1.0, 1): 1.4142135623730951, (1.0, 100): 0.1414213562373095, (1.0, 1024): 0.044194173824159223,
    (1.0, 4096): 0.022097086912079612, (2.5, 1): 2.2360679774997898, (2.5, 100): 0.22360679774997896,
    (2.5, 1024): 0.069877124296868431, (2.5, 4096): 0.034938562148434216, (0.37, 1): 0.86023252670426265,
    (0.37, 100): 0.086023252670426265, (0.37, 1024): 0.026882266459508208, (0.37, 4096): 0.013441133229754104,
}
DEFAULT_MAX_ITER = 15000


def mismatches(plan):
    """Every row of the tables above that the compiled header answers differently."""
    bad = []
    bad += [("block", k) for k, v in BLOCK_ROWS.items() if plan.block(*k) != v]
    bad += [("ns", S) for S, v in NS_ROWS.items() if plan.L.ns(S) != v]
    bad += [("threads", M) for M, v in THREAD_ROWS.items() if plan.L.threads(M) != v]
    bad += [("scale", k) for k, v in SCALE_ROWS.items() if plan.L.scale(*k) != v]
    bad += [("max_iter",)] if plan.L.default_max_iter() != DEFAULT_MAX_ITER else []
    return bad


def test_the_tables(plan):
    assert set(BLOCK_ROWS) <= {(S, F, N, NP, d, R) for S, F, (N, NP), d, R in GRID}
    assert mismatches(plan) == []


def test_the_block_over_the_whole_grid(plan):
    """From the arrays' own sizes, in bytes: every region starts where the one before it ends (status and evals: R ints of slack
    behind each), the block ends where the last one does."""
    for S, F, (N, NP), d, R in GRID:
        b = dict(zip(FIELDS, plan.block(S, F, N, NP, d, R)))
        da = d if R else 0
        sizes = [("omega", 8 * F * d), ("phase", 8 * F), ("weights", 8 * S * F), ("eps", 8 * S * N), ("G", 8 * S * NP),
                 ("T", 8 * S * NP), ("V", 8 * S * NP), ("lo", 8 * da), ("hi", 8 * da), ("starts", 8 * R * d), ("x", 8 * R * d),
                 ("g", 8 * R * d), ("f", 8 * R), ("start_idx", 8 * R), ("status", 4 * R + 4 * R), ("evals", 4 * R + 4 * R)]
        at = 0
        for name, n in sizes:
            assert b[name] * (4 if name in ("status", "evals") else 8) == at, (name, S, F, N, d, R)
            at += n
        assert at == 8 * b["doubles"]
        # what the code relies on, said directly
        assert (8 * b["start_idx"]) % 8 == 0 and b["status"] % 2 == 0 and b["evals"] % 2 == 0      # int64s, then ints from a double's start
        assert b["status"] + R <= b["evals"] and b["evals"] + R <= 2 * b["doubles"]
        assert b["doubles"] - b["lo"] == (2 * d + 3 * R * d + 4 * R if R else 0)                     # the old path_ascent_doubles
        assert b["lo"] == F * d + F + S * F + S * N + 3 * S * NP


def test_the_dispatch_rules_on_both_sides_of_their_edges(plan):
    assert [plan.L.ns(S) for S in (1, 2, 4, 5, 16)] == [1, 4, 4, 16, 16]
    assert [plan.L.threads(M) for M in (2**17 - 1, 2**17)] == [64, 256]
    assert plan.L.default_max_iter() == 15000


MOVED = [   # one constant or term each
    ("S == 1 ? 1", "S == 2 ? 1"), ("S <= 4 ? 4", "S <= 5 ? 4"), ("PATH_EVAL_WIDE_M = 1 << 17", "PATH_EVAL_WIDE_M = (1 << 17) + 1"),
    ("? 256u : 64u", "? 256u : 128u"), ("2.0 * amplitude", "1.0 * amplitude"),
    ("PATH_DEFAULT_MAX_ITER = 15000", "PATH_DEFAULT_MAX_ITER = 15001"), ("b.omega + F * d", "b.omega + F * d + 1"),
    ("b.phase + F;", "b.phase + F + 1;"), ("b.weights + S * F", "b.weights + S * F + 1"), ("b.eps + S * N;", "b.eps + S * N + 1;"),
    ("b.G + S * NP", "b.G + S * NP + 1"), ("b.T + S * NP", "b.T + S * NP + 1"), ("b.V + S * NP", "b.V + S * NP + 1"),
    ("b.lo + da", "b.lo + da + 1"), ("b.hi + da", "b.hi + da + 1"), ("b.starts + R * d", "b.starts + R * d + 1"),
    ("b.x + R * d", "b.x + R * d + 1"), ("b.g + R * d", "b.g + R * d + 1"), ("b.f + R;", "b.f + R + 1;"),
    ("2 * (b.start_idx + R)", "2 * (b.start_idx + R) + 1"), ("2 * (b.f + 3 * R)", "2 * (b.f + 3 * R) + 1"),
    ("b.f + 4 * R", "b.f + 4 * R + 1"),
]


@pytest.mark.parametrize("old,new", MOVED, ids=["ns_1", "ns_4", "wide_m", "threads", "scale", "max_iter", "phase", "weights", "eps", "G",
                                                "T", "V", "lo", "hi", "starts", "x", "g", "f", "start_idx", "status", "evals",
                                                "doubles"])
def test_a_moved_constant_changes_a_row(tmp_path, old, new):
    src = open(os.path.join(CSRC, "path_plan.h")).read()
    assert src.count(old) == 1, old
    with open(tmp_path / "path_plan.h", "w") as f:
        f.write(src.replace(old, new))
    assert mismatches(Plan(str(tmp_path), header_dir=str(tmp_path))) != []
