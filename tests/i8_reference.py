"""Host reference of the int8 posterior GEMM (bayesianoptimization_amd/csrc/posterior_i8.hip), in NumPy and Python integers.
Imports nothing from the package: every function is written from the scheme's description, not from the code it judges.

Scheme (S = 7 digit planes).  An operand x, |x| <= 1, is rounded once to Q = rint(x 2^(8S-2)) (ties to even) and Q is written in
balanced base 256, Q = sum_t b_t 256^(S-1-t), b_1 ... b_{S-1} in [-128, 127], b_0 what is left.  Row i of W is divided by 2^e_i
first (e_i = frexp exponent of its largest magnitude), k* is taken as it is.  The GEMM keeps the digit products (s, t) with
s + t <= S - 1 and sums those of one level l = s + t into one integer L_l per output; the value of an output is
    v_i = (sum_l L_l 256^(2S-2-l)) 2^(e_i - 2 (8S-2)).
Per 128-row chunk and candidate the kernel then adds v_i^2 in a fixed order (order_model_part).

Operand buffers, both in fragment order: [block of 16 items][64-step][plane][lane 16 g + item] 16 bytes, an item a row of W or a
candidate, a 64-step 64 consecutive train points, lane 16 g + item holding the item's digits of the train points 16 g ... 16 g + 15
of the step, one per byte.  A block of candidates holds all NP / 64 steps; the block b of rows 16 b ... 16 b + 15 of the lower
triangular W holds the steps 0 ... b / 4 only, the blocks one after the other without padding.

The only compiled pieces are elementwise primitives with no structure of their own (shim()): a true fused multiply-add (the
interpreter's math.fma where it exists) and the header's i8_combine, which tests/test_int8_digits_host.py pins to exact arithmetic
and which the ORDER model may use; the exact-value functions use integers only."""
import ctypes
import math
import os
import shutil
import subprocess
import tempfile
from fractions import Fraction

import numpy as np

S = 7
F = 8 * S - 2                      # fraction bits of a quantised operand
ROWS = 128                         # rows of W per workgroup (chunk) of the GEMM
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bayesianoptimization_amd", "csrc")


# ---- quantisation and digits ------------------------------------------------------------------------------------------
def quantize(x):
    """Q = rint(x 2^(8S-2)), ties to even, as int64 (the scaling by a power of two is exact, np.rint rounds to even)."""
    x = np.asarray(x, dtype=np.float64)
    assert np.all(np.abs(x) <= 1.0)
    return np.rint(np.ldexp(x, F)).astype(np.int64)


def digits(Q):
    """Balanced base-256 digits of Q: array [S, ...] int8, plane 0 the leading digit."""
    Q = np.asarray(Q, dtype=np.int64).copy()
    out = np.empty((S,) + Q.shape, dtype=np.int8)
    for t in range(S - 1, 0, -1):
        b = ((Q + 128) & 255) - 128            # in [-128, 127], congruent to Q mod 256
        out[t] = b
        Q = (Q - b) >> 8                       # exact: Q - b is a multiple of 256
    assert np.all(np.abs(Q) <= 65), "leading digit out of range: |x| > 1?"
    out[0] = Q
    return out


def undigits(D):
    """Q from digit planes [S, ...] (any int8 digits, legal or not)."""
    Q = np.zeros(D.shape[1:], dtype=np.int64)
    for t in range(S):
        Q = Q * 256 + D[t].astype(np.int64)
    return Q


def row_exponents(W, N):
    """frexp exponent of max_j<=i |W_ij| over the N x N lower triangle; 0 for an all-zero row and for rows >= N."""
    NP = W.shape[0]
    e = np.zeros(NP, dtype=np.int64)
    for i in range(min(N, NP)):
        mx = float(np.max(np.abs(W[i, :i + 1])))
        e[i] = math.frexp(mx)[1] if mx > 0.0 else 0
    return e


def w_quantized(W, N, e):
    """Q of every entry of W's N x N lower triangle scaled by 2^-e_i, zero elsewhere: [NP, NP] int64."""
    NP = W.shape[0]
    Wl = np.zeros_like(W)
    Wl[:N, :N] = np.tril(W[:N, :N])
    return quantize(np.ldexp(Wl, (-np.asarray(e, dtype=np.int64)).astype(np.int32)[:, None]))


def scale_of_exponent(e):
    """The power of two that turns the combined level sums (units of the lowest kept level, 256^(S-1)) into v."""
    return np.ldexp(1.0, (np.asarray(e, dtype=np.int64) - 2 * F + 8 * (S - 1)).astype(np.int32))


# ---- packing ------------------------------------------------------------------------------------------------------------
def wd_steps(nb):
    """First 64-step of each of the nb blocks of 16 rows in the W buffer, and the total: block b holds b // 4 + 1 steps."""
    n = np.arange(nb) // 4 + 1
    first = np.concatenate(([0], np.cumsum(n)))
    return first[:-1], int(first[-1])


def wd_bytes(NP):
    return wd_steps(NP // 16)[1] * S * 64 * 16


def pack_w(D):
    """Digit planes of W [S, NP, NP] int8 -> the W buffer (int8, flat).  Only the steps a block holds are stored."""
    NP = D.shape[1]
    first, total = wd_steps(NP // 16)
    buf = np.zeros((total, S, 4, 16, 16), dtype=np.int8)           # [step][plane][g][item][byte]
    for b in range(NP // 16):
        n = b // 4 + 1
        blk = D[:, 16 * b:16 * b + 16, :64 * n].reshape(S, 16, n, 4, 16)   # [plane][item][step][g][byte]
        buf[first[b]:first[b] + n] = blk.transpose(2, 0, 3, 1, 4)
    return buf.reshape(-1)


def unpack_w(buf, NP):
    """The W buffer -> digit planes [S, NP, NP] int8 (zero where the buffer holds no step)."""
    first, total = wd_steps(NP // 16)
    buf = np.asarray(buf, dtype=np.int8).reshape(total, S, 4, 16, 16)
    D = np.zeros((S, NP, NP), dtype=np.int8)
    for b in range(NP // 16):
        n = b // 4 + 1
        D[:, 16 * b:16 * b + 16, :64 * n] = buf[first[b]:first[b] + n].transpose(1, 3, 0, 2, 4).reshape(S, 16, 64 * n)
    return D


def pack_k(D):
    """Digit planes of k* [S, M, NP] int8 (M a multiple of 16) -> the k* buffer: [block][step][plane][g][item][byte]."""
    _, M, NP = D.shape
    blk = D.reshape(S, M // 16, 16, NP // 64, 4, 16)                # [plane][block][item][step][g][byte]
    return np.ascontiguousarray(blk.transpose(1, 3, 0, 4, 2, 5)).reshape(-1)


def unpack_k(buf, M, NP):
    buf = np.asarray(buf, dtype=np.int8).reshape(M // 16, NP // 64, S, 4, 16, 16)
    return np.ascontiguousarray(buf.transpose(2, 0, 4, 1, 3, 5)).reshape(S, M, NP)


# ---- exact level sums and values ----------------------------------------------------------------------------------------
def level_sums(A, B):
    """L[l] = sum_{s+t=l} A_s B_t^T for l <= S - 1: [S, NP, M] int64 from A [S, NP, NP] (the stored part of W: whatever lies in
    the buffer is multiplied) and B [S, M, NP].  fp64 BLAS, exact: every |a b| <= 2^14 and a level has at most S NP terms."""
    NP = A.shape[1]
    assert S * 128 * 128 * NP < 2 ** 53, "fp64 sums of the digit products would not be exact"
    assert S * 128 * 128 * NP < 2 ** 31, "the kernel's int32 level sums would overflow"
    L = np.zeros((S, NP, B.shape[1]))
    Bt = [np.ascontiguousarray(B[t].T, dtype=np.float64) for t in range(S)]
    for s in range(S):
        As = A[s].astype(np.float64)
        for t in range(S - s):
            L[s + t] += As @ Bt[t]
    Li = L.astype(np.int64)
    assert np.array_equal(Li, L) and np.max(np.abs(Li)) < 2 ** 31
    return Li


def exact_units(L):
    """U = sum_l L_l 256^(2S-2-l) as Python integers (object array [NP, M]): v_i = U_i 2^(e_i - 2 (8S-2))."""
    U = np.zeros(L.shape[1:], dtype=object)
    for l in range(S):
        U = U + L[l].astype(object) * (256 ** (2 * S - 2 - l))
    return U


def exact_v(L, e):
    """v as Fractions [NP, M] (small cases)."""
    U = exact_units(L)
    out = np.empty(U.shape, dtype=object)
    for i in range(U.shape[0]):
        sc = Fraction(2) ** int(e[i] - 2 * F)
        for j in range(U.shape[1]):
            out[i, j] = U[i, j] * sc
    return out


def exact_part(L, e):
    """sum of v_i^2 over each 128-row chunk, exact: [ceil(NP / 128), M] Fractions."""
    NP, M = L.shape[1:]
    U = exact_units(L)
    x = [int(v) - 2 * F for v in e]
    xmin = min(x)
    sq = U * U
    for i in range(NP):
        sq[i] = sq[i] * (4 ** (x[i] - xmin))
    unit = Fraction(4) ** xmin
    nch = (NP + ROWS - 1) // ROWS
    out = np.empty((nch, M), dtype=object)
    for r in range(nch):
        tot = sq[ROWS * r:ROWS * (r + 1)].sum(axis=0)
        for j in range(M):
            out[r, j] = tot[j] * unit
    return out


# ---- elementwise primitives ---------------------------------------------------------------------------------------------
_SHIM_SRC = r"""
#include <cmath>
#include "i8_digits.h"
using namespace gpbo;
extern "C" {
int s_digits() { return I8_S; }
// out[i] = fma(v[i], v[i], s[i]), one rounding (std::fma is never split)
void fma_sq(const double* v, const double* s, double* out, int64_t n) { for (int64_t i = 0; i < n; ++i) out[i] = std::fma(v[i], v[i], s[i]); }
void combine_n(const int32_t* acc, double* out, int64_t n) { for (int64_t i = 0; i < n; ++i) out[i] = i8_combine<I8_S>(acc + i * I8_S); }
int64_t frag_index(int64_t first_step, int64_t k, int plane, int item) { return i8_frag_index<I8_S>(first_step, k, plane, item); }
int64_t kd_block(int64_t cb, int64_t NP) { return i8_kd_block(cb, NP); }
int64_t wd_block(int64_t b) { return i8_wd_block(b); }
}
"""
_shim = None


def shim():
    """The header's i8_combine / index functions and std::fma for the host (compiled once per process)."""
    global _shim
    if _shim is None:
        cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
        if cxx is None:
            raise RuntimeError("no host C++ compiler")
        with tempfile.TemporaryDirectory(prefix="i8ref") as d:   # the loaded library outlives its file
            src, so = os.path.join(d, "shim.cpp"), os.path.join(d, "libi8ref.so")
            with open(src, "w") as f:
                f.write(_SHIM_SRC)
            subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I" + CSRC, src, "-o", so], check=True)
            L = ctypes.CDLL(so)
        i64, pd = ctypes.c_int64, ctypes.POINTER(ctypes.c_double)
        L.fma_sq.argtypes = [pd, pd, pd, i64]
        L.fma_sq.restype = None
        L.combine_n.argtypes = [ctypes.POINTER(ctypes.c_int32), pd, i64]
        L.combine_n.restype = None
        L.frag_index.restype = L.kd_block.restype = L.wd_block.restype = i64
        L.frag_index.argtypes = [i64, i64, ctypes.c_int, ctypes.c_int]
        L.kd_block.argtypes = [i64, i64]
        L.wd_block.argtypes = [i64]
        assert L.s_digits() == S
        _shim = L
    return _shim


def fma_sq(v, s):
    """fma(v, v, s) elementwise with ONE rounding."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    s = np.ascontiguousarray(s, dtype=np.float64)
    assert v.shape == s.shape
    if hasattr(math, "fma"):
        return np.array([math.fma(a, a, b) for a, b in zip(v.ravel(), s.ravel())]).reshape(v.shape)
    out = np.empty_like(v)
    pd = ctypes.POINTER(ctypes.c_double)
    shim().fma_sq(v.ctypes.data_as(pd), s.ctypes.data_as(pd), out.ctypes.data_as(pd), v.size)
    return out


def combine(L):
    """i8_combine of the level sums [S, ...] -> fp64 in units of the lowest kept level."""
    acc = np.ascontiguousarray(np.moveaxis(L, 0, -1), dtype=np.int32)
    out = np.empty(acc.shape[:-1])
    shim().combine_n(acc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), out.size)
    return out


# ---- the order model ----------------------------------------------------------------------------------------------------
def order_model_part(L, wscale):
    """part [ceil(NP / 128), M] in the kernel's summation order.  v = combine(levels) * wscale (one product by a power of two); per
    wave (32 rows) and candidate two fma chains s = fma(v, v, s) from 0 over the rows 4 h + {0-3, 8-11, 16-19, 24-27}, h = 0, 1;
    half 0 + half 1; the chunk's four waves ((w0 + w1) + w2) + w3, a wave without rows (ragged last chunk) counting 0.0."""
    NP, M = L.shape[1:]
    v = combine(L) * np.asarray(wscale, dtype=np.float64)[:, None]
    V = v.reshape(NP // 32, 32, M)
    half = []
    for h in (0, 1):
        s = np.zeros((NP // 32, M))
        for base in (0, 8, 16, 24):
            for i in range(4):
                s = fma_sq(V[:, 4 * h + base + i, :], s)
        half.append(s)
    nch = (NP + ROWS - 1) // ROWS
    waves = np.zeros((nch * 4, M))
    waves[:NP // 32] = half[0] + half[1]
    w = waves.reshape(nch, 4, M)
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


# Error bound of a chunk's sum against exact_part, in units of 2^-53 times the exact sum.  Every term is non-negative.
#   * v: within 1 ulp of its exact value (i8_combine's contract; the product by the row's power of two is exact), i.e. a relative
#     error of at most 2^-52, so v^2 is off by at most (2 + 2^-52) 2^-52 < 4.000001 * 2^-53 of itself;
#   * the sum: an output passes through 16 fma (one chain of 16 rows), 1 add (half 0 + half 1) and 3 adds (four waves): 20
#     roundings, each at most 2^-53 of a partial sum that never exceeds the (perturbed) total.
# (4 + 20) 2^-53, and one more unit for the second-order terms (24^2 2^-106 and the like): 25.
PART_BOUND_UNITS = 25


def part_error_units(part, exact):
    """max over the outputs of |part - exact| / (2^-53 exact) (0 where both are 0; inf where only exact is)."""
    worst = 0.0
    for p, x in zip(np.asarray(part).ravel(), exact.ravel()):
        if not math.isfinite(p):
            return math.inf
        d = abs(Fraction(float(p)) - x)
        if d:
            worst = max(worst, float(d / x * 2 ** 53) if x else math.inf)
    return worst
