"""CPU: the fixed-point int8 digit split of the posterior's int8 GEMM (bayesianoptimization_amd/csrc/i8_digits.h), compiled
for the host with the system C++ compiler and checked against exact integer / rational arithmetic in Python:

  * the digits of a quantised value reconstruct it exactly, and the quantisation is within half a unit of 2^-(8S-2);
  * every digit is an int8, the leading one within [-65, 65];
  * the int32 level sums cannot overflow at the largest NP the kernel serves, with every digit at -128;
  * the fp64 epilogue (i8_combine) is within 2 ulp of the exact value of the truncated digit product.

Inputs: random rows, rows spanning 1e-12 ... 1e4 (W of an ill-conditioned fit), k* = 1.0, tiny k* and k* = 0."""
import ctypes
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "bayesianoptimization_amd", "csrc")

SHIM = r"""
#include "i8_digits.h"
using namespace gpbo;
extern "C" {
int s_digits() { return I8_S; }
int np_max() { return I8_NP_MAX; }
int64_t quantize(double x) { return i8_quantize<I8_S>(x); }
int64_t offset() { return i8_offset<I8_S>(); }
int digit(int64_t qo, int t) { return (int)(int8_t)(uint8_t)i8_digit_byte<I8_S>(qo, t); }
int row_exponent(double m) { return i8_row_exponent(m); }
double combine(const int32_t* acc) { return i8_combine<I8_S>(acc); }
int scale_exp(int e) { return i8_scale_exp<I8_S>(e); }
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("i8")
    src, so = d / "shim.cpp", d / "libi8.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + CSRC, str(src), "-o", str(so)], check=True)
    L = ctypes.CDLL(str(so))
    L.quantize.restype = ctypes.c_int64
    L.quantize.argtypes = [ctypes.c_double]
    L.offset.restype = ctypes.c_int64
    L.digit.argtypes = [ctypes.c_int64, ctypes.c_int]
    L.row_exponent.argtypes = [ctypes.c_double]
    L.combine.restype = ctypes.c_double
    L.combine.argtypes = [ctypes.POINTER(ctypes.c_int32)]
    L.scale_exp.argtypes = [ctypes.c_int]
    return L


def _digits(lib, x):
    S = lib.s_digits()
    qo = lib.quantize(x)
    return qo - lib.offset(), [lib.digit(qo, t) for t in range(S)]


def _rows():
    rng = np.random.RandomState(5)
    yield rng.uniform(-1.0, 1.0, 200)
    yield np.sign(rng.standard_normal(200)) * 10.0 ** rng.uniform(-12, 4, 200)   # 1e-12 ... 1e4 in one row
    yield np.array([1.0, -1.0, 0.5, 2.0 ** -60, -(2.0 ** -60), 0.0, 1.0 - 2.0 ** -53, 3.0])


def test_digits_reconstruct_their_input(lib):
    S = lib.s_digits()
    F = 8 * S - 2
    for row in _rows():
        e = lib.row_exponent(float(np.max(np.abs(row))))
        for x in row:
            xs = float(np.ldexp(x, -e))
            assert abs(xs) < 1.0
            q, dg = _digits(lib, xs)
            assert sum(b * 256 ** (S - 1 - t) for t, b in enumerate(dg)) == q
            assert all(-128 <= b <= 127 for b in dg[1:]) and -65 <= dg[0] <= 65
            assert abs(Fraction(xs) - Fraction(q, 2 ** F)) <= Fraction(1, 2 ** (F + 1))
    for k in (1.0, 0.0, 1e-300, 2.0 ** -57, 0.3, 1.0 - 2.0 ** -53):     # k* in [0, 1]: no scale
        q, dg = _digits(lib, k)
        assert sum(b * 256 ** (S - 1 - t) for t, b in enumerate(dg)) == q
        assert abs(Fraction(k) - Fraction(q, 2 ** F)) <= Fraction(1, 2 ** (F + 1))
    assert _digits(lib, 1.0)[0] == 2 ** F                                 # 1.0 exact


def test_level_sums_stay_in_int32(lib):
    S, NP = lib.s_digits(), lib.np_max()
    worst = S * 128 * 128 * NP                                           # level S-1 holds S products per train point
    assert worst < 2 ** 31


def test_epilogue_is_within_two_ulp_of_the_exact_sum(lib):
    S = lib.s_digits()
    rng = np.random.RandomState(9)
    cases = [rng.randint(-2 ** 31, 2 ** 31, S) for _ in range(3000)]
    cases += [np.full(S, -2 ** 31 + 1), np.full(S, 2 ** 31 - 1), np.zeros(S, dtype=np.int64)]
    cases += [np.array([1] + [0] * (S - 2) + [-1]), np.array([0] * (S - 1) + [1])]
    cancel = []                                                          # heavy cancellation between levels
    for c in cases[:500]:
        c2 = np.array(c, dtype=np.int64)
        c2[S - 1] = -int(c2[S - 2] % 2 ** 23) * 256
        c2[S - 2] = c2[S - 2] % 2 ** 23
        cancel.append(c2)
    for c in cases + cancel:
        acc = (ctypes.c_int32 * S)(*[int(v) for v in c])
        got = lib.combine(acc)
        exact = sum(int(v) * 256 ** (S - 1 - l) for l, v in enumerate(c))
        if exact == 0:
            assert got == 0.0
            continue
        ulp = np.spacing(abs(float(exact)))
        assert abs(Fraction(got) - exact) <= 2 * Fraction(ulp), (list(c), got, exact)


def test_scale_exponent_maps_the_lowest_level_to_v(lib):
    """v = combine(acc) * 2^scale_exp(e): the lowest kept level, 256^(S-1) in units of 2^-(16S-4), times the row's 2^e."""
    S = lib.s_digits()
    for e in (-20, 0, 11):
        assert lib.scale_exp(e) == e - (16 * S - 4) + 8 * (S - 1)
