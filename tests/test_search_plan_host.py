"""CPU: how the one-launch searches are served and laid out (bayesianoptimization_amd/csrc/search_plan.h), compiled for the host
with the system C++ compiler and checked against the tables written out below, on both sides of every edge:

  * the local searches' mode (W in LDS | W in memory | not served), dynamic-LDS bytes and X staging at NP = 64, 128 | 192 and
    512 | 576 for d at both ends of every padded width, with GPBO_POLISH_FUSED_MAX_NP at 0, 128, 512 and above 512, and on both
    sides of every d at which X stops fitting;
  * the evolution's mode, whether its population sits in LDS, and its bytes, for S in {5, 75, 960, 1024} x D in {1, 5, 64} and on
    both sides of every S at which the population stops fitting (mode never changes along S: W in LDS beside the largest
    population's energies and index array still fits at NP = 128), the analytic objective (no model), the switch, and the
    evaluations per launch at 128 | 192 and 256 | 320;
  * both LDS layouts: arrays in order, back to back, 16-byte aligned where the kernels rely on it, ending at the reported total;
  * both host / device blocks: regions in order, back to back, ints behind the doubles, ending at the reported bytes.

The tables were printed once from a verbatim copy of the rules as they stood in polish_fused.hip and evolve.hip before the header
existed (33 135 371 cases compared, no difference).  A constant of the header moved by one step changes at least one row
(test_a_moved_constant_changes_a_row moves each)."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "bayesianoptimization_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")

SHIM = r"""
#include "search_plan.h"
using namespace gpbo;
extern "C" {
int no_override() { return NO_OVERRIDE; }
int max_np(int override_) { return search_max_np(override_); }
void polish(int NP, int d, int DP, int override_, int* out) {
  const PolishPlan p = plan_polish(NP, d, DP, override_);
  out[0] = (int)p.mode; out[1] = p.lds_bytes; out[2] = p.x_staged;
}
int one_launch(int n_constraints, int mode, const char* sw) { return polish_one_launch(n_constraints, (SearchMode)mode, sw); }
void polish_layout(int NP, int d, int DP, int wlds, int* o) {
  const PolishLds l = polish_lds(NP, d, DP, wlds != 0);
  const int v[] = {l.W, l.xs, l.ls, l.alpha, l.ks, l.vs, l.cc, l.pp, l.us, l.red, l.opt, l.X, l.flag, l.x_doubles, l.bytes};
  for (int i = 0; i < 15; ++i) o[i] = v[i];
}
void evolve(int NP, int S, int D, int override_, int analytic, int* out) {
  const EvolvePlan p = plan_evolve(NP, S, D, override_, analytic != 0);
  out[0] = (int)p.mode; out[1] = p.pop_lds; out[2] = p.lds_bytes; out[3] = p.evals_per_launch;
}
void evolve_layout(int NP, int S, int D, int wlds, int pop, int* o) {
  const EvolveLds l = evolve_lds(NP, S, D, wlds != 0, pop != 0);
  const int v[] = {l.W, l.xs, l.ls, l.px, l.ks, l.vs, l.pp, l.E, l.misc, l.acc, l.pop, l.key, l.perm, l.frames, l.bytes};
  for (int i = 0; i < 15; ++i) o[i] = v[i];
}
void polish_blk(int S, int d, size_t* o) {
  const PolishBlock b = polish_block(S, d);
  const size_t v[] = {b.seeds, b.lo, b.hi, b.x, b.f, b.dbg, b.ints, b.status, b.iter, b.evals, b.bytes};
  for (int i = 0; i < 11; ++i) o[i] = v[i];
}
void evolve_blk(int S, int D, int eval_n, size_t* o) {
  const EvolveBlock b = evolve_block(S, D, eval_n);
  const size_t v[] = {b.pop, b.E, b.arg1, b.arg2, b.aw, b.aa, b.eval_x, b.eval_out, b.scale, b.ints,
                      b.ist, b.perm, b.ckind, b.cg0, b.cgn, b.key, b.bytes};
  for (int i = 0; i < 17; ++i) o[i] = v[i];
}
}
"""

MODES = ["NotServed", "WInLds", "WInMemory"]                                     # enum class SearchMode, by value
POLISH_LDS = ["W", "xs", "ls", "alpha", "ks", "vs", "cc", "pp", "us", "red", "opt", "X", "flag", "x_doubles", "bytes"]
EVOLVE_LDS = ["W", "xs", "ls", "px", "ks", "vs", "pp", "E", "misc", "acc", "pop", "key", "perm", "frames", "bytes"]
POLISH_BLK = ["seeds", "lo", "hi", "x", "f", "dbg", "ints", "status", "iter", "evals", "bytes"]
EVOLVE_BLK = ["pop", "E", "arg1", "arg2", "aw", "aa", "eval_x", "eval_out", "scale", "ints", "ist", "perm", "ckind", "cg0", "cgn",
              "key", "bytes"]


def pad_dim(d):
    return next(p for p in (4, 8, 16, 32, 64) if d <= p)


class Plan:
    def __init__(self, tmp_dir, header_dir=CSRC):
        cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
        if cxx is None:
            pytest.fail("no host C++ compiler")
        src, so = os.path.join(tmp_dir, "shim.cpp"), os.path.join(tmp_dir, "libsearchplan.so")
        with open(src, "w") as f:
            f.write(SHIM)
        # the copied header first, the tree's fit_plan.h (NO_OVERRIDE) behind it
        subprocess.run([cxx, "-std=c++17", "-O1", "-fPIC", "-shared", "-I" + header_dir, "-I" + CSRC, "-I" + INCLUDE, src, "-o", so],
                       check=True)
        L = self.L = ctypes.CDLL(so)
        L.one_launch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p]
        self.unset = L.no_override()

    def _ov(self, v):
        return self.unset if v is None else v

    def _ints(self, fn, n, *args):
        out = (ctypes.c_int * n)()
        fn(*args, out)
        return list(out)

    def _sizes(self, fn, names, *args):
        out = (ctypes.c_size_t * len(names))()
        fn(*args, out)
        return dict(zip(names, out))

    def polish(self, NP, d, override=None):
        m, b, st = self._ints(self.L.polish, 3, NP, d, pad_dim(d), self._ov(override))
        return MODES[m], b, bool(st)

    def evolve(self, NP, S, D, override=None, analytic=False):
        m, pop, b, budget = self._ints(self.L.evolve, 4, NP, S, D, self._ov(override), int(analytic))
        return MODES[m], bool(pop), b, budget

    def polish_layout(self, NP, d, wlds):
        return dict(zip(POLISH_LDS, self._ints(self.L.polish_layout, 15, NP, d, pad_dim(d), int(wlds))))

    def evolve_layout(self, NP, S, D, wlds, pop):
        return dict(zip(EVOLVE_LDS, self._ints(self.L.evolve_layout, 15, NP, S, D, int(wlds), int(pop))))

    def polish_block(self, S, d):
        return self._sizes(self.L.polish_blk, POLISH_BLK, S, d)

    def evolve_block(self, S, D, eval_n):
        return self._sizes(self.L.evolve_blk, EVOLVE_BLK, S, D, eval_n)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return Plan(str(tmp_path_factory.mktemp("search_plan")))


# ---- the local searches.  (NP, d) -> (mode, dynamic-LDS bytes, X staged); DP = pad_dim(d), the switch not set
POLISH_ROWS = {
    (64, 1): ("WInLds", 42736, True), (64, 4): ("WInLds", 43216, True), (64, 5): ("WInLds", 45296, True), (64, 8): ("WInLds", 45776, True),
    (64, 9): ("WInLds", 49968, True), (64, 16): ("WInLds", 51088, True), (64, 17): ("WInLds", 59408, True),
    (64, 32): ("WInLds", 61808, True), (64, 33): ("WInLds", 78336, True), (64, 64): ("WInLds", 83296, True),
    (128, 1): ("WInLds", 149488, True), (128, 4): ("WInLds", 149968, True), (128, 5): ("WInLds", 153968, True), (128, 8): ("WInLds", 154448, True),
    (128, 9): ("WInLds", 162672, True), (128, 16): ("WInLds", 163792, True), (128, 17): ("WInLds", 146480, False),
    (128, 32): ("WInLds", 148880, False), (128, 33): ("WInLds", 149008, False), (128, 64): ("WInLds", 153968, False),
    (192, 1): ("WInMemory", 25328, True), (192, 4): ("WInMemory", 25808, True), (192, 5): ("WInMemory", 31728, True), (192, 8): ("WInMemory", 32208, True),
    (192, 9): ("WInMemory", 44464, True), (192, 16): ("WInMemory", 45584, True), (192, 17): ("WInMemory", 70224, True),
    (192, 32): ("WInMemory", 72624, True), (192, 33): ("WInMemory", 121888, True), (192, 64): ("WInMemory", 126848, True),
    (512, 1): ("WInMemory", 65008, True), (512, 4): ("WInMemory", 65488, True), (512, 5): ("WInMemory", 81008, True), (512, 8): ("WInMemory", 81488, True),
    (512, 9): ("WInMemory", 113904, True), (512, 16): ("WInMemory", 115024, True), (512, 17): ("WInMemory", 45296, False),
    (512, 32): ("WInMemory", 47696, False), (512, 33): ("WInMemory", 47728, False), (512, 64): ("WInMemory", 52688, False),
    (576, 1): ("NotServed", 0, False), (576, 4): ("NotServed", 0, False), (576, 5): ("NotServed", 0, False), (576, 8): ("NotServed", 0, False),
    (576, 9): ("NotServed", 0, False), (576, 16): ("NotServed", 0, False), (576, 17): ("NotServed", 0, False),
    (576, 32): ("NotServed", 0, False), (576, 33): ("NotServed", 0, False), (576, 64): ("NotServed", 0, False),
}
# both sides of every d at which X stops fitting: (NP, d) -> (bytes, X staged)
STAGE_EDGE_ROWS = {
    (128, 16): (163792, True), (128, 17): (146480, False), (256, 54): (163664, True), (256, 55): (30704, False),
    (320, 32): (116720, True), (320, 33): (32320, False), (384, 32): (138768, True), (384, 33): (37456, False),
    (448, 32): (160816, True), (448, 33): (42592, False), (512, 16): (115024, True), (512, 17): (45296, False),
}
# (NP, GPBO_POLISH_FUSED_MAX_NP, mode) at d = 4
POLISH_OVERRIDE_ROWS = [
    (64, 0, "NotServed"), (128, 0, "NotServed"), (192, 0, "NotServed"), (512, 0, "NotServed"), (576, 0, "NotServed"),
    (64, 128, "WInLds"), (128, 128, "WInLds"), (192, 128, "NotServed"), (512, 128, "NotServed"), (576, 128, "NotServed"),
    (64, 512, "WInLds"), (128, 512, "WInLds"), (192, 512, "WInMemory"), (512, 512, "WInMemory"), (576, 512, "NotServed"),
    (64, 576, "WInLds"), (128, 576, "WInLds"), (192, 576, "WInMemory"), (512, 576, "WInMemory"), (576, 576, "NotServed"),
    (64, 1024, "WInLds"), (128, 1024, "WInLds"), (192, 1024, "WInMemory"), (512, 1024, "WInMemory"), (576, 1024, "NotServed"),
]
# ---- the evolution.  (NP, S, D) -> (mode, population in LDS, dynamic-LDS bytes); the switch not set
EVOLVE_ROWS = {
    (64, 5, 1): ("WInLds", True, 39844), (64, 5, 5): ("WInLds", True, 40004), (64, 5, 64): ("WInLds", True, 42364),
    (64, 75, 1): ("WInLds", True, 41244), (64, 75, 5): ("WInLds", True, 43644), (64, 75, 64): ("WInLds", True, 79044),
    (64, 960, 1): ("WInLds", True, 58944), (64, 960, 5): ("WInLds", True, 89664), (64, 960, 64): ("WInLds", False, 51264),
    (64, 1024, 1): ("WInLds", True, 60224), (64, 1024, 5): ("WInLds", True, 92992), (64, 1024, 64): ("WInLds", False, 52032),
    (128, 5, 1): ("WInLds", True, 140708), (128, 5, 5): ("WInLds", True, 140868), (128, 5, 64): ("WInLds", True, 143228),
    (128, 75, 1): ("WInLds", True, 142108), (128, 75, 5): ("WInLds", True, 144508), (128, 75, 64): ("WInLds", False, 141508),
    (128, 960, 1): ("WInLds", True, 159808), (128, 960, 5): ("WInLds", False, 152128), (128, 960, 64): ("WInLds", False, 152128),
    (128, 1024, 1): ("WInLds", True, 161088), (128, 1024, 5): ("WInLds", False, 152896), (128, 1024, 64): ("WInLds", False, 152896),
    (192, 5, 1): ("WInMemory", True, 10660), (192, 5, 5): ("WInMemory", True, 10820), (192, 5, 64): ("WInMemory", True, 13180),
    (192, 75, 1): ("WInMemory", True, 12060), (192, 75, 5): ("WInMemory", True, 14460), (192, 75, 64): ("WInMemory", True, 49860),
    (192, 960, 1): ("WInMemory", True, 29760), (192, 960, 5): ("WInMemory", True, 60480), (192, 960, 64): ("WInMemory", False, 22080),
    (192, 1024, 1): ("WInMemory", True, 31040), (192, 1024, 5): ("WInMemory", True, 63808), (192, 1024, 64): ("WInMemory", False, 22848),
    (512, 5, 1): ("WInMemory", True, 20900), (512, 5, 5): ("WInMemory", True, 21060), (512, 5, 64): ("WInMemory", True, 23420),
    (512, 75, 1): ("WInMemory", True, 22300), (512, 75, 5): ("WInMemory", True, 24700), (512, 75, 64): ("WInMemory", True, 60100),
    (512, 960, 1): ("WInMemory", True, 40000), (512, 960, 5): ("WInMemory", True, 70720), (512, 960, 64): ("WInMemory", False, 32320),
    (512, 1024, 1): ("WInMemory", True, 41280), (512, 1024, 5): ("WInMemory", True, 74048), (512, 1024, 64): ("WInMemory", False, 33088),
    (576, 5, 1): ("NotServed", False, 0), (576, 5, 5): ("NotServed", False, 0), (576, 5, 64): ("NotServed", False, 0),
    (576, 75, 1): ("NotServed", False, 0), (576, 75, 5): ("NotServed", False, 0), (576, 75, 64): ("NotServed", False, 0),
    (576, 960, 1): ("NotServed", False, 0), (576, 960, 5): ("NotServed", False, 0), (576, 960, 64): ("NotServed", False, 0),
    (576, 1024, 1): ("NotServed", False, 0), (576, 1024, 5): ("NotServed", False, 0), (576, 1024, 64): ("NotServed", False, 0),
}
# both sides of every S at which the population stops fitting (NP = 0: the analytic objective)
EVOLVE_EDGE_ROWS = {
    (0, 304, 64): ("WInMemory", True, 163712), (0, 305, 64): ("WInMemory", False, 8076),
    (64, 236, 64): ("WInLds", True, 163408), (64, 237, 64): ("WInLds", False, 42588),
    (128, 446, 5): ("WInLds", True, 163800), (128, 447, 5): ("WInLds", False, 145972),
    (128, 44, 64): ("WInLds", True, 163664), (128, 45, 64): ("WInLds", False, 141148),
    (192, 292, 64): ("WInMemory", True, 163568), (192, 293, 64): ("WInMemory", False, 14076),
    (512, 272, 64): ("WInMemory", True, 163328), (512, 273, 64): ("WInMemory", False, 24076),
}
# the analytic objective (no model, W nowhere: the kernel's W-in-memory instance): (S, D) -> (population in LDS, bytes)
ANALYTIC_ROWS = {
    (5, 1): (True, 4516), (5, 5): (True, 4676), (5, 64): (True, 7036),
    (75, 1): (True, 5916), (75, 5): (True, 8316), (75, 64): (True, 43716),
    (960, 1): (True, 23616), (960, 5): (True, 54336), (960, 64): (False, 15936),
    (1024, 1): (True, 24896), (1024, 5): (True, 57664), (1024, 64): (False, 16704),
}
# (NP, GPBO_POLISH_FUSED_MAX_NP, mode) at S = 75, D = 5: the switch moves the evolution's limit too
EVOLVE_OVERRIDE_ROWS = [
    (64, 0, "NotServed"), (128, 0, "NotServed"), (192, 0, "NotServed"), (512, 0, "NotServed"), (576, 0, "NotServed"),
    (64, 128, "WInLds"), (128, 128, "WInLds"), (192, 128, "NotServed"), (512, 128, "NotServed"), (576, 128, "NotServed"),
    (64, 512, "WInLds"), (128, 512, "WInLds"), (192, 512, "WInMemory"), (512, 512, "WInMemory"), (576, 512, "NotServed"),
    (64, 576, "WInLds"), (128, 576, "WInLds"), (192, 576, "WInMemory"), (512, 576, "WInMemory"), (576, 576, "NotServed"),
    (64, 1024, "WInLds"), (128, 1024, "WInLds"), (192, 1024, "WInMemory"), (512, 1024, "WInMemory"), (576, 1024, "NotServed"),
]
# NP -> evaluations per launch
BUDGET_ROWS = {64: 384, 128: 384, 192: 96, 256: 96, 320: 48, 512: 48 }
# (n_seeds, d) -> bytes of the local searches' pinned block
PINNED_BYTES = {(1, 1): 108, (1, 5): 332, (1, 64): 3636, (10, 1): 936, (10, 5): 2600, (10, 64): 27144, (64, 1): 5904, (64, 5): 16208, (64, 64): 168192 }


def mismatches(plan):
    """Every row of the tables above that the compiled header answers differently."""
    bad = []
    bad += [("polish", k) for k, v in POLISH_ROWS.items() if plan.polish(*k) != v]
    bad += [("stage", k) for k, v in STAGE_EDGE_ROWS.items() if plan.polish(*k)[1:] != v]
    bad += [("polish override", r) for r in POLISH_OVERRIDE_ROWS if plan.polish(r[0], 4, r[1])[0] != r[2]]
    bad += [("evolve", k) for k, v in EVOLVE_ROWS.items() if plan.evolve(*k)[:3] != v]
    bad += [("evolve edge", k) for k, v in EVOLVE_EDGE_ROWS.items() if plan.evolve(*k, analytic=k[0] == 0)[:3] != v]
    bad += [("analytic", k) for k, v in ANALYTIC_ROWS.items() if plan.evolve(512, *k, analytic=True)[:3] != ("WInMemory",) + v]
    bad += [("evolve override", r) for r in EVOLVE_OVERRIDE_ROWS if plan.evolve(r[0], 75, 5, r[1])[0] != r[2]]
    bad += [("budget", NP) for NP, v in BUDGET_ROWS.items() if plan.evolve(NP, 75, 5)[3] != v]
    bad += [("pinned", k) for k, v in PINNED_BYTES.items() if plan.polish_block(*k)["bytes"] != v]
    return bad


def test_the_tables(plan):
    assert mismatches(plan) == []


def test_the_cap_both_searches_share(plan):
    assert [plan.L.max_np(plan._ov(v)) for v in (None, 0, 64, 128, 512, 576, 4096, -64)] == [512, 0, 64, 128, 512, 512, 512, -64]
    # the analytic objective has no model: whatever the switch and the slot's size say
    for ov in (None, 0, 128, -64):
        assert plan.evolve(4096, 75, 5, ov, analytic=True)[:3] == ("WInMemory",) + ANALYTIC_ROWS[(75, 5)]


def test_one_launch_needs_one_served_model_and_the_switch_not_off(plan):
    one = lambda n_c, mode, sw: bool(plan.L.one_launch(n_c, MODES.index(mode), sw))
    assert one(0, "WInLds", None) and one(0, "WInMemory", None) and one(0, "WInLds", b"1") and one(0, "WInLds", b"")
    assert not one(0, "NotServed", None) and not one(1, "WInLds", None) and not one(0, "WInLds", b"0") and not one(0, "WInMemory", b"01")


def _check_back_to_back(off, sizes, unit, total):
    """`sizes`: [(name, length)] in layout order, lengths and offsets in bytes: every array starts where the one before it ends."""
    at = 0
    for name, n in sizes:
        assert off[name] * unit[name] == at, name
        at += n
    assert at == total


def test_polish_lds_layout(plan):
    """The largest images too: NP = 128 with d = DP = 64 in LDS (19 244 doubles before X), NP = 512 streamed (6 584)."""
    for NP in (64, 128, 192, 256, 512):
        for d in (1, 4, 5, 8, 9, 16, 17, 32, 33, 54, 55, 64):
            for wlds in ([True, False] if NP <= 128 else [False]):
                DP = pad_dim(d)
                l = plan.polish_layout(NP, d, wlds)
                want = NP * (DP + 1)
                assert l["x_doubles"] == (want if l["X"] + want <= 160 * 128 - 8 else 0)
                sizes = [("W", NP * (NP + 1) if wlds else 0), ("xs", 64), ("ls", 64), ("alpha", NP), ("ks", NP), ("vs", NP), ("cc", 2 * NP),
                         ("pp", 2 * NP), ("us", NP), ("red", (64 // DP) * (NP // 64) * (2 * DP + 2)), ("opt", 20 * d + 40),
                         ("X", l["x_doubles"])]
                _check_back_to_back(l, [(n, 8 * s) for n, s in sizes] + [("flag", 16)], dict.fromkeys(POLISH_LDS, 8), l["bytes"])
                # pr_smem is aligned(16): the (c1, c2) / (v^2, k* alpha) pairs and the two-rows-per-thread stores into vs / us are 16-byte units
                assert all(l[n] % 2 == 0 for n, _ in sizes) and l["flag"] % 2 == 0
                assert l["bytes"] <= 160 * 1024
    assert plan.polish_layout(128, 64, True)["X"] == 19244 and plan.polish_layout(512, 64, False)["X"] == 6584


def test_evolve_lds_layout(plan):
    for NP in (0, 64, 128, 192, 512):
        for S in (5, 44, 45, 75, 960, 1024):
            for D in (1, 5, 64):
                for wlds in ([True, False] if 0 < NP <= 128 else [False]):
                    for pop in (True, False):
                        l = plan.evolve_layout(NP, S, D, wlds, pop)
                        doubles = [("W", NP * (NP + 1) if wlds else 0), ("xs", 64), ("ls", 64), ("px", 64), ("ks", NP), ("vs", NP),
                                   ("pp", 2 * NP), ("E", S), ("misc", 8), ("acc", 16), ("pop", S * D if pop else 0)]
                        ints = [("key", 624), ("perm", S), ("frames", 3 * 16)]
                        unit = {**dict.fromkeys(EVOLVE_LDS, 8), "key": 4, "perm": 4, "frames": 4}
                        _check_back_to_back(l, [(n, 8 * s) for n, s in doubles] + [(n, 4 * s) for n, s in ints], unit, l["bytes"])
                        # ev_smem is aligned(16): vs and pp take pairs; everything up to E sits on 16 bytes whatever S and D are
                        assert all(l[n] % 2 == 0 for n in ("W", "xs", "ls", "px", "ks", "vs", "pp", "E"))
                        assert l["key"] % 2 == 0      # the ints start on a double's boundary


def test_the_blocks(plan):
    for S in (1, 10, 64):
        for d in (1, 5, 64):
            b = plan.polish_block(S, d)
            sizes = [("seeds", S * d), ("lo", d), ("hi", d), ("x", S * d), ("f", S), ("dbg", S * (4 + 3 * d)), ("ints", 0)]
            unit = {**dict.fromkeys(POLISH_BLK, 8), "status": 4, "iter": 4, "evals": 4}
            _check_back_to_back(b, [(n, 8 * s) for n, s in sizes] + [(n, 4 * S) for n in ("status", "iter", "evals")], unit, b["bytes"])
    for S in (5, 75, 1024):
        for D in (1, 5, 64):
            for n in (0, 1, 7):
                b = plan.evolve_block(S, D, n)
                sizes = [("pop", S * D), ("E", S), ("arg1", D), ("arg2", D), ("aw", D), ("aa", D), ("eval_x", n * D), ("eval_out", n),
                         ("scale", 1), ("ints", 0)]
                ints = [("ist", 8), ("perm", S), ("ckind", D), ("cg0", D), ("cgn", D), ("key", 624)]
                unit = {**dict.fromkeys(EVOLVE_BLK, 8), **dict.fromkeys([k for k, _ in ints], 4)}
                _check_back_to_back(b, [(k, 8 * s) for k, s in sizes] + [(k, 4 * s) for k, s in ints], unit, b["bytes"])


MOVED = [   # one constant each: the size limits by one 64-step, the LDS budget by 1 KiB, the flag words by one pair
    ("SEARCH_LDS_NP = 128", "SEARCH_LDS_NP = 64"), ("SEARCH_MAX_NP = 512", "SEARCH_MAX_NP = 576"),
    ("SEARCH_NP_DEFAULT = 512", "SEARCH_NP_DEFAULT = 448"), ("SEARCH_LDS_BYTES = 160 * 1024", "SEARCH_LDS_BYTES = 159 * 1024"),
    ("SEARCH_LDS_BYTES / 8 - 8", "SEARCH_LDS_BYTES / 8 - 10"), ("NP <= 128 ? 384", "NP <= 192 ? 384"), ("(NP <= 256 ? 96 : 48)", "(NP <= 320 ? 96 : 48)"),
    ("POLISH_OPT_PAIRS = 10", "POLISH_OPT_PAIRS = 11"), ("EV_STACK = 16", "EV_STACK = 17"),
]


@pytest.mark.parametrize("old,new", MOVED, ids=["lds_np", "max_np", "np_default", "lds_bytes", "x_cap", "budget_128", "budget_256",
                                                "opt_pairs", "ev_stack"])
def test_a_moved_constant_changes_a_row(tmp_path, old, new):
    src = open(os.path.join(CSRC, "search_plan.h")).read()
    assert src.count(old) == 1, old
    with open(tmp_path / "search_plan.h", "w") as f:
        f.write(src.replace(old, new))
    assert mismatches(Plan(str(tmp_path), header_dir=str(tmp_path))) != []
