"""CPU: the posterior's path rule (bayesianoptimization_amd/csrc/posterior_plan.h, plan_posterior), compiled for the host with
the system C++ compiler and checked against the rule written out below as a table, on both sides of every edge:

  * NP across the row-chunk, Fused512, int8 and fp32-MFMA edges; Mp across the four batch edges of two row chunks, each
    reached from M = Mp and from M = Mp - 127 (the same padded batch);
  * M at the GEMV limit and one above it, with GPBO_POST_SMALL=0 and without, fp32 and fp64;
  * every GPBO_POST_KERNEL digit over the whole grid (2, 3 always; 4 up to NP = 1024; 8 for 512 < NP <= 16384; fp64 only);
  * the partial-row counts the finalize kernel sums and whether a fused kernel writes mu / sd itself;
  * the slab paths' slab (slab_spec): bytes per candidate, offset cap and whether a slab below 128 candidates is allowed, and
    the size of the slab buffer (slab_doubles) against the three expressions it replaced.

A threshold of the header moved by one step (64 in NP, 128 in Mp) changes at least one row of the grid."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "bayesianoptimization_amd", "csrc")

SHIM = r"""
#include "posterior_plan.h"
extern "C" void plan(int64_t NP, int64_t M, int f32, int64_t lim, int force, int no_small, int no_fuse, int* out) {
  const gpbo::PostPlan p = gpbo::plan_posterior(NP, M, f32 != 0, lim, force, no_small != 0, no_fuse != 0);
  out[0] = (int)p.path; out[1] = p.fuse_ends; out[2] = p.part_chunks; out[3] = p.mu_chunks;
}
extern "C" void spec(int path, int64_t NP, int64_t* out) {
  const gpbo::SlabSpec s = gpbo::slab_spec((gpbo::PostPath)path, NP);
  out[0] = s.bytes_per_cand; out[1] = s.offset_cap; out[2] = s.narrow_ok;
}
extern "C" int64_t slab_doubles(int64_t ms, int64_t bytes_per_cand) { return gpbo::slab_doubles(ms, bytes_per_cand); }
extern "C" int i8_s() { return gpbo::I8_S; }
"""

PATHS = ["Small", "Fused256", "Fused512", "SlabF64", "SlabI8", "SlabF32"]   # enum class PostPath, in order

NPS = [256, 320, 384, 448, 512, 576, 1024, 1088, 1984, 2048, 16384, 16448]
MPS = [8064, 8192, 9088, 9216, 16384, 16512, 32640, 32768]


def build_plan(tmp_dir, include_dir=CSRC):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src, so = os.path.join(tmp_dir, "shim.cpp"), os.path.join(tmp_dir, "libplan.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-fPIC", "-shared", "-I" + include_dir, src, "-o", so], check=True)
    L = ctypes.CDLL(so)
    L.plan.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                       ctypes.POINTER(ctypes.c_int)]

    L.spec.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    L.slab_doubles.argtypes = [ctypes.c_int64, ctypes.c_int64]
    L.slab_doubles.restype = ctypes.c_int64

    def plan(NP, M, f32, lim, force=0, no_small=False, no_fuse=False):
        out = (ctypes.c_int * 4)()
        L.plan(NP, M, int(f32), lim, force, int(no_small), int(no_fuse), out)
        return PATHS[out[0]], bool(out[1]), out[2], out[3]

    def spec(path, NP):
        out = (ctypes.c_int64 * 3)()
        L.spec(PATHS.index(path), NP, out)
        return out[0], out[1], bool(out[2])

    plan.spec, plan.slab_doubles, plan.i8_s = spec, L.slab_doubles, L.i8_s()
    return plan


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return build_plan(str(tmp_path_factory.mktemp("plan")))


def _ceil(a, b):
    return -(-a // b)


def expected(NP, M, f32, lim, force=0, no_small=False, no_fuse=False):
    """The rule as a table: the first row that matches wins."""
    nchunks, Mp = _ceil(NP, 256), _ceil(M, 128) * 128
    if M <= lim and not no_small:
        return "Small", False, 0, 0
    if f32:
        return "SlabF32", False, (_ceil(NP, 512) if NP >= 512 else nchunks), nchunks
    if NP <= 256:
        path = "Fused256"
    elif NP <= 512:
        path = ("Fused256" if Mp < 8192 else "SlabF64" if Mp < 9216 else "Fused512" if Mp <= 16384 else
                "Fused256" if Mp < 32768 else "Fused512" if NP >= 384 else "SlabF64")
    else:
        path = "SlabI8" if 2048 <= NP <= 16384 else "SlabF64"
    if force in (2, 3):
        path = {2: "Fused256", 3: "SlabF64"}[force]
    elif force == 4 and NP <= 1024:
        path = "Fused512"
    elif force == 8 and 512 < NP <= 16384:
        path = "SlabI8"
    part = {"Fused256": nchunks, "SlabF64": nchunks, "Fused512": _ceil(NP, 512), "SlabI8": _ceil(NP, 128)}[path]
    mu = 1 if path.startswith("Fused") else nchunks
    fuse = not no_fuse and ((path == "Fused256" and NP <= 256) or (path == "Fused512" and NP <= 512))
    return path, fuse, part, mu


def test_batch_and_size_edges(plan):
    for NP, Mp, f32, no_fuse in itertools.product(NPS, MPS, (False, True), (False, True)):
        for M in (Mp, Mp - 127):
            assert plan(NP, M, f32, 48, no_fuse=no_fuse) == expected(NP, M, f32, 48, no_fuse=no_fuse), (NP, M, f32, no_fuse)


def test_gemv_limit(plan):
    for NP, lim, f32, no_small in itertools.product(NPS, (48, 128, 512, 1024), (False, True), (False, True)):
        for M in (lim, lim + 1):
            got = plan(NP, M, f32, lim, no_small=no_small)
            assert got == expected(NP, M, f32, lim, no_small=no_small), (NP, M, lim, f32, no_small)
            assert (got[0] == "Small") == (M == lim and not no_small)
        # an override never bypasses the GEMV path
        assert plan(NP, lim, False, lim, force=8)[0] == "Small"


def test_every_override_digit(plan):
    for NP, Mp, f32, force in itertools.product(NPS, MPS, (False, True), range(10)):
        assert plan(NP, Mp, f32, 48, force=force) == expected(NP, Mp, f32, 48, force=force), (NP, Mp, f32, force)
    # the bounds of 4 and 8 in the grid above, spelled out
    assert plan(1024, 128, False, 0, force=4)[:3] == ("Fused512", False, 2)
    assert plan(1088, 128, False, 0, force=4)[0] == "SlabF64"
    assert plan(512, 128, False, 0, force=4)[:2] == ("Fused512", True)
    assert plan(512, 128, False, 0, force=8)[0] == "Fused256"
    assert plan(576, 128, False, 0, force=8)[0] == "SlabI8"
    assert plan(16448, 128, False, 0, force=8)[0] == "SlabF64"
    assert plan(4096, 128, True, 0, force=8)[0] == "SlabF32"


def test_headline_configs(plan):
    """The benchmark configurations, as literal rows (C3: N = 4096 at 2^20 candidates; C1: N = 256; C2: N = 512 at 65 536;
    C5: fp32)."""
    assert plan(4096, 1 << 20, False, 128) == ("SlabI8", False, 32, 16)
    assert plan(256, 10000, False, 48) == ("Fused256", True, 1, 1)
    assert plan(512, 65536, False, 48) == ("Fused512", True, 1, 1)
    assert plan(512, 65536, False, 48, no_fuse=True) == ("Fused512", False, 1, 1)
    assert plan(1024, 1 << 20, True, 512) == ("SlabF32", False, 2, 4)
    assert plan(448, 1 << 20, True, 48) == ("SlabF32", False, 2, 2)


def test_slab_spec_of_the_three_slab_paths(plan):
    """bytes per candidate 8 NP / 4 NP / I8_S NP; three rows of a stage as 32-bit buffer offsets cap the value slabs at 80e6 / 160e6
    candidates, the int8 slab has no cap; only the int8 walk may run a slab below 128 candidates."""
    assert plan.i8_s == 7
    for NP in (64, 640, 2048, 16384):
        assert plan.spec("SlabF64", NP) == (8 * NP, 80 * 1000 * 1000, False)
        assert plan.spec("SlabF32", NP) == (4 * NP, 160 * 1000 * 1000, False)
        assert plan.spec("SlabI8", NP) == (7 * NP, 2**63 - 1, True)
        assert 3 * 8 * plan.spec("SlabF64", NP)[1] < 2**31 and 3 * 4 * plan.spec("SlabF32", NP)[1] < 2**31


def test_slab_buffer_size_equals_the_three_former_expressions(plan):
    """The slab buffer is counted in doubles.  (ms * bytes_per_cand + 7) / 8 is ms * NP for fp64, (ms * NP + 1) / 2 for fp32 — odd
    products included: NP is a multiple of 64 on the device, the rule itself does not need it — and (ms * 7 NP + 7) / 8 for int8."""
    for ms, NP in itertools.product((1, 3, 127, 128, 129, 384, 8191, 8192, 121984, 80 * 1000 * 1000), (1, 63, 64, 65, 320, 577, 640, 2048, 16384)):
        assert plan.slab_doubles(ms, 8 * NP) == ms * NP
        assert plan.slab_doubles(ms, 4 * NP) == (ms * NP + 1) // 2
        assert plan.slab_doubles(ms, 7 * NP) == (ms * NP * 7 + 7) // 8
        for bpc in (8 * NP, 4 * NP, 7 * NP):
            assert 8 * plan.slab_doubles(ms, bpc) >= ms * bpc > 8 * (plan.slab_doubles(ms, bpc) - 1)
