"""CPU: the slab width of the int8 posterior's walk (bayesianoptimization_amd/csrc/posterior_plan.h, i8_slab_width), compiled for the
host with the system C++ compiler and checked against literal tables: per NP the width under the 256 MB bound whose generation
grid (ceil(width / 256) x ceil(NP / 256) workgroups) fills the largest share of its last round over the device's compute units (256 on an MI355X), and what
a granted width (the workspace budget's, a multiple of 128, at most the padded batch) makes of it, on both sides of each edge."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "bayesianoptimization_amd", "csrc")

SHIM = r"""
#include "posterior_plan.h"
extern "C" int64_t width(int64_t NP, int64_t bytes_per_cand, int64_t granted, int64_t cus) {
  return gpbo::i8_slab_width(NP, bytes_per_cand, granted, cus);
}
"""

S = 7   # digit planes: bytes per candidate = NP * S
ALL = 1 << 40


@pytest.fixture(scope="module")
def width(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    tmp = str(tmp_path_factory.mktemp("i8w"))
    src, so = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "libi8w.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-fPIC", "-shared", "-I" + CSRC, src, "-o", so], check=True)
    L = ctypes.CDLL(so)
    L.width.argtypes = [ctypes.c_int64] * 4
    L.width.restype = ctypes.c_int64
    return lambda NP, granted=ALL, bytes_per_cand=None, cus=256: L.width(NP, bytes_per_cand or NP * S, granted, cus)


# NP: (width, candidates that fit 256e6 B, generation workgroups = width / 256 * ceil(NP / 256))
RULE = {
    1536: (21760, 23809, 510),
    2048: (16384, 17857, 512),     # exactly two rounds
    2112: (14336, 17316, 504),     # 9 chunks: 57 x 9 = 513 would start a third round
    3072: (10752, 11904, 504),
    4096: (8192, 8928, 512),       # C3: 8832 would be 35 x 16 = 560 workgroups, 0.73 of three rounds
    4160: (7680, 8791, 510),
    8192: (4096, 4464, 512),
    16384: (2048, 2232, 512),
}


def test_width_per_np(width):
    for NP, (w, fit, wgs) in RULE.items():
        assert 256_000_000 // (NP * S) == fit and w <= fit < 2 * w and w % 256 == 0
        assert w // 256 * -(-NP // 256) == wgs and wgs <= 512
        assert width(NP) == w, NP


def test_no_wider_width_fills_better(width):
    """Among the multiples of 256 from half the byte bound up to it, none fills its last round better, and no wider one as well."""
    for NP, (w, fit, wgs) in RULE.items():
        chunks = -(-NP // 256)
        fill = lambda k: k * chunks / (-(-k * chunks // 256) * 256)
        kmax = fit // 256
        for k in range(kmax // 2 + 1, kmax + 1):
            assert fill(k) <= fill(w // 256) and (k <= w // 256 or fill(k) < fill(w // 256)), (NP, k)


def test_granted_width_edges(width):
    """A budget or a batch below the rule's width is taken as it is (at least 128); at and above it the rule's width holds."""
    for NP, rows in {4096: [(0, 128), (128, 128), (3072, 3072), (8064, 8064), (8192, 8192), (8320, 8192), (8832, 8192), (1 << 20, 8192)],
                     2048: [(128, 128), (6912, 6912), (16256, 16256), (16384, 16384), (16512, 16384), (100096, 16384)],
                     16384: [(128, 128), (1920, 1920), (2048, 2048), (2176, 2048), (3072, 2048)]}.items():
        for granted, want in rows:
            assert width(NP, granted) == want, (NP, granted)


def test_fewer_than_256_candidates_fit(width):
    """A candidate of more than a 256th of the byte bound (no NP the int8 GEMM serves): the plain multiple of 128, at least 128."""
    assert width(16384, ALL, 1_500_000) == 128
    assert width(16384, ALL, 3_000_000) == 128
    assert width(16384, ALL, 900_000) == 256     # 284 fit: one unit of 256


def test_other_compute_unit_counts(width):
    """The rule fills the device it is told about, not an MI355X's 256 units."""
    assert width(4096, cus=304) == 4864     # 19 x 16 = 304 workgroups: one round
    assert width(2048, cus=304) == 9728     # 38 x 8 = 304
    assert width(4096, cus=128) == 8192     # 512 = four rounds
    assert width(4096, cus=32) == 8704      # 34 x 16 = 544 = 17 rounds: the widest that fills
    assert width(16384, cus=304) == 2048    # 8 x 64 = 512 of 608: nothing under the byte bound does better
