"""CPU: the operand layout of the int8 posterior GEMM on v_mfma_i32_16x16x64_i8 (bayesianoptimization_amd/csrc/i8_digits.h:
i8_frag_index, i8_kd_block, i8_wd_block — the functions wd_pack_kernel, kstar_gen_kernel's digit branch and the GEMM address
their buffers with), compiled for the host:

  * over every (block of 16 items, 16 train points, plane, item) that a pack kernel writes, the 16-byte fragment index is a
    bijection onto the buffer — the k* slab of a few candidate blocks and the lower-triangle W — for NP = 64, 2112, 4096;
  * a fragment is [block][64-step][plane][lane], lane 16 g + item for the train points 16 g ... 16 g + 15 of the step;
  * i8_wd_block counts, per block of 16 rows, exactly the 64-steps that hold a part of the lower triangle (no padding steps:
    the kernel writes the steps 0 ... b / 4 of block b and nothing else), and a wave's two 16-row blocks hold the same steps."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "bayesianoptimization_amd", "csrc")

SHIM = r"""
#include "i8_digits.h"
using namespace gpbo;
extern "C" {
int s_digits() { return I8_S; }
int64_t frag_index(int64_t first_step, int64_t k, int plane, int item) { return i8_frag_index<I8_S>(first_step, k, plane, item); }
int64_t kd_block(int64_t cb, int64_t NP) { return i8_kd_block(cb, NP); }
int64_t wd_block(int64_t b) { return i8_wd_block(b); }
// every fragment wd_pack_kernel writes (block b, steps 0 ... b / 4); returns how many, -1 if one lies outside [0, size)
int64_t cover_w(int64_t NP, int32_t* hits, int64_t size) {
  int64_t n = 0;
  for (int64_t b = 0; b < NP / 16; ++b)
    for (int64_t k = 0; k < 64 * (b / 4 + 1); k += 16)
      for (int p = 0; p < I8_S; ++p)
        for (int r = 0; r < 16; ++r, ++n) {
          const int64_t i = i8_frag_index<I8_S>(i8_wd_block(b), k, p, r);
          if (i < 0 || i >= size) return -1;
          ++hits[i];
        }
  return n;
}
// every fragment kstar_gen_kernel writes for ncb blocks of 16 candidates
int64_t cover_k(int64_t NP, int64_t ncb, int32_t* hits, int64_t size) {
  int64_t n = 0;
  for (int64_t cb = 0; cb < ncb; ++cb)
    for (int64_t k = 0; k < NP; k += 16)
      for (int p = 0; p < I8_S; ++p)
        for (int r = 0; r < 16; ++r, ++n) {
          const int64_t i = i8_frag_index<I8_S>(i8_kd_block(cb, NP), k, p, r);
          if (i < 0 || i >= size) return -1;
          ++hits[i];
        }
  return n;
}
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("i8layout")
    src, so = d / "shim.cpp", d / "libi8layout.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + CSRC, str(src), "-o", str(so)], check=True)
    L = ctypes.CDLL(str(so))
    i64, p32 = ctypes.c_int64, ctypes.POINTER(ctypes.c_int32)
    L.frag_index.restype = i64
    L.frag_index.argtypes = [i64, i64, ctypes.c_int, ctypes.c_int]
    L.kd_block.restype = i64
    L.kd_block.argtypes = [i64, i64]
    L.wd_block.restype = i64
    L.wd_block.argtypes = [i64]
    for f in (L.cover_w, L.cover_k):
        f.restype = i64
    L.cover_w.argtypes = [i64, p32, i64]
    L.cover_k.argtypes = [i64, i64, p32, i64]
    return L


def _hits(size):
    h = np.zeros(size, dtype=np.int32)
    return h, h.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


@pytest.mark.parametrize("NP", [64, 2112, 4096])
def test_fragment_index_is_a_bijection_onto_both_buffers(lib, NP):
    S = lib.s_digits()
    size_w = lib.wd_block(NP // 16) * S * 64             # what pack_wd allocates, in 16-byte fragments
    h, p = _hits(size_w)
    assert lib.cover_w(NP, p, size_w) == size_w and np.all(h == 1)
    ncb = 12                                              # 192 candidates: NP * S bytes each
    size_k = ncb * 16 * NP * S // 16
    h, p = _hits(size_k)
    assert lib.cover_k(NP, ncb, p, size_k) == size_k and np.all(h == 1)


def test_fragment_order_is_block_step_plane_lane(lib):
    S = lib.s_digits()
    for first, k, plane, item in ((0, 0, 0, 0), (5, 63, 6, 15), (17, 64 * 9 + 37, 3, 7), (1 << 20, 16383, 2, 11)):
        lane = 16 * ((k % 64) // 16) + item
        assert lib.frag_index(first, k, plane, item) == ((first + k // 64) * S + plane) * 64 + lane
    assert lib.kd_block(7, 2112) == 7 * 33


@pytest.mark.parametrize("NP", [64, 2112, 4096, 16384])
def test_wd_block_counts_the_steps_of_the_lower_triangle(lib, NP):
    total = 0
    for b in range(NP // 16):
        assert lib.wd_block(b) == total
        # 64-steps with a column <= the block's last row; the pack kernel writes exactly these (ks <= b / 4), no padding step
        steps = sum(1 for ks in range(NP // 64) if 64 * ks <= 16 * b + 15)
        assert steps == b // 4 + 1
        total += steps
    assert lib.wd_block(NP // 16) == total
    for rb in range(NP // 32):                             # a wave: blocks 2 rb, 2 rb + 1, both rb / 2 + 1 steps, adjacent
        n = rb // 2 + 1
        assert lib.wd_block(2 * rb + 1) - lib.wd_block(2 * rb) == n == lib.wd_block(2 * rb + 2) - lib.wd_block(2 * rb + 1)
