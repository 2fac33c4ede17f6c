"""CPU: the host reference of the int8 posterior GEMM (tests/i8_reference.py) is validated here before
tests/test_gpu_int8_exact.py lets it judge a kernel:

  * pack -> unpack of both operand buffers is the identity, and the W buffer stores nothing but the lower triangle's steps;
  * the byte the packers put an element at is the one the header's i8_frag_index / i8_wd_block / i8_kd_block name (host shim);
  * the digits reconstruct Q, Q is rint with ties to even;
  * the BLAS level sums and the exact v equal a brute-force product in Python integers / Fractions at NP = 64 and 128;
  * the order model equals an independent straight-line evaluation: the kernel's epilogue replayed lane by lane, with the three
    cross-lane moves and the two legs every lane runs, on fused multiply-adds done in rational arithmetic."""
from fractions import Fraction

import numpy as np
import pytest

import i8_reference as R

S = R.S


def _random_operands(NP, M, seed, lower=True):
    rng = np.random.RandomState(seed)
    A = rng.randint(-128, 128, size=(S, NP, NP)).astype(np.int8)
    if lower:
        A *= np.tril(np.ones((NP, NP), dtype=np.int8))[None]
    B = rng.randint(-128, 128, size=(S, M, NP)).astype(np.int8)
    return A, B


@pytest.mark.parametrize("NP", [64, 192, 2112])
def test_pack_unpack_round_trip(NP):
    M = 48
    A, B = _random_operands(NP, M, NP, lower=False)
    buf = R.pack_w(A)
    assert buf.dtype == np.int8 and buf.size == R.wd_bytes(NP)
    stored = np.zeros((NP, NP), dtype=bool)                 # what the buffer holds: per 16-row block the steps up to the diagonal's
    for b in range(NP // 16):
        stored[16 * b:16 * b + 16, :64 * (b // 4 + 1)] = True
    assert np.array_equal(R.unpack_w(buf, NP), A * stored[None])
    assert np.array_equal(R.pack_w(R.unpack_w(buf, NP)), buf)
    kb = R.pack_k(B)
    assert kb.size == M * NP * S
    assert np.array_equal(R.unpack_k(kb, M, NP), B)
    assert np.array_equal(R.pack_k(R.unpack_k(kb, M, NP)), kb)


@pytest.mark.parametrize("NP", [64, 2112])
def test_packers_put_every_element_where_the_header_says(NP):
    sh = R.shim()
    rng = np.random.RandomState(3)
    M = 48
    # one element at a time: a buffer with a single non-zero byte, found at 16 * fragment index + (train point mod 16)
    for _ in range(40):
        plane, row = int(rng.randint(S)), int(rng.randint(NP))
        col = int(rng.randint(64 * (row // 64 + 1)))        # inside the steps the row's block holds
        A = np.zeros((S, NP, NP), dtype=np.int8)
        A[plane, row, col] = 77
        (at,) = np.nonzero(R.pack_w(A))
        assert list(at) == [16 * sh.frag_index(sh.wd_block(row // 16), col, plane, row % 16) + col % 16]
        cand, k = int(rng.randint(M)), int(rng.randint(NP))
        B = np.zeros((S, M, NP), dtype=np.int8)
        B[plane, cand, k] = -5
        (at,) = np.nonzero(R.pack_k(B))
        assert list(at) == [16 * sh.frag_index(sh.kd_block(cand // 16, NP), k, plane, cand % 16) + k % 16]
    first, total = R.wd_steps(NP // 16)
    assert [sh.wd_block(b) for b in range(NP // 16)] == list(first) and sh.wd_block(NP // 16) == total


def test_the_engine_wrappers_size_their_buffers_as_the_header_does():
    """GpEngine.debug_i8_* allocate the host buffers the library writes: their S and W-buffer size are the header's."""
    from bayesianoptimization_amd.engine import GpEngine

    sh = R.shim()
    assert GpEngine.I8_S == sh.s_digits() == S
    for NP in (64, 128, 192, 2048, 2112, 4096, 16384):
        assert GpEngine._i8_wd_bytes(NP) == sh.wd_block(NP // 16) * S * 64 * 16 == R.wd_bytes(NP)


def test_quantisation_and_digits():
    x = np.array([1.0, -1.0, 0.0, 2.0 ** -54, 2.0 ** -55, 3 * 2.0 ** -55, -(2.0 ** -55), 0.3, 1.0 - 2.0 ** -53, 2.0 ** -60])
    Q = R.quantize(x)
    assert list(Q[:7]) == [2 ** 54, -(2 ** 54), 0, 1, 0, 2, 0]            # ties to even: 0.5 -> 0, 1.5 -> 2, -0.5 -> 0
    for xv, q in zip(x, Q):
        assert abs(Fraction(float(xv)) * 2 ** R.F - int(q)) <= Fraction(1, 2)
    rng = np.random.RandomState(1)
    Q = np.concatenate((Q, R.quantize(rng.uniform(-1, 1, 1000))))
    D = R.digits(Q)
    assert np.array_equal(R.undigits(D), Q)
    assert np.all(np.abs(D[0].astype(int)) <= 65)


@pytest.mark.parametrize("NP,M", [(64, 16), (128, 4)])
def test_level_sums_and_exact_v_against_brute_force(NP, M):
    A, B = _random_operands(NP, M, 10 + NP)
    e = np.random.RandomState(NP).randint(-30, 31, size=NP)
    L = R.level_sums(A, B)
    V = R.exact_v(L, e)
    a, b = A.astype(int).tolist(), B.astype(int).tolist()
    for i in range(NP):
        for j in range(M):
            lv = [0] * S
            for s in range(S):
                for t in range(S - s):
                    lv[s + t] += sum(x * y for x, y in zip(a[s][i], b[t][j]))
            assert lv == [int(L[l, i, j]) for l in range(S)]
            # the truncated product of the two fixed-point numbers sum_s a_s 256^-s 2^-(8S-2) 256^(S-1) ...: digit s of an operand
            # weighs 256^(S-1-s) 2^-(8S-2)
            v = sum(Fraction(lv[l]) * Fraction(256) ** (2 * S - 2 - l) for l in range(S)) / Fraction(4) ** R.F * Fraction(2) ** int(e[i])
            assert V[i, j] == v
    P = R.exact_part(L, e)
    for r in range(NP // 128 or 1):
        for j in range(M):
            assert P[r, j] == sum(V[i, j] ** 2 for i in range(128 * r, min(NP, 128 * (r + 1))))


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))      # int / int division rounds correctly: one rounding


def _lane_replay(L, wscale, NP, M):
    """posterior_i8_kernel's epilogue and `part` sum, lane by lane: lane 16 g + c of wave w holds, for the candidate block j and
    the 16-row tile a, the rows 32 w + 16 a + 4 g + i (i = 0 ... 3) of candidate 16 j + c."""
    v = R.combine(L) * np.asarray(wscale)[:, None]
    nch = (NP + 127) // 128
    part = np.zeros((nch, M))
    for r in range(nch):
        for ct in range(M // 64):
            red = np.zeros((4, 64))
            for wave in range(4):
                rb = 4 * r + wave
                ss = np.zeros((4, 64))                               # [j][lane]
                if rb < NP // 32:
                    for j in range(4):
                        s = [0.0] * 64
                        for a in range(2):
                            vv = [[v[32 * rb + 16 * a + 4 * (lane >> 4) + i, 64 * ct + 16 * j + (lane & 15)] for i in range(4)]
                                  for lane in range(64)]
                            for lane in range(64):
                                for i in range(4):
                                    s[lane] = _fma(vv[lane][i], vv[lane][i], s[lane])
                            s = [s[lane ^ 32] for lane in range(64)]
                            for lane in range(64):
                                for i in range(4):
                                    s[lane] = _fma(vv[lane][i], vv[lane][i], s[lane])
                            if a == 0:
                                s = [s[lane ^ 32] for lane in range(64)]
                        ss[j] = s
                for j in range(4):
                    for lane in range(32, 48):                        # lane group 2 writes half 0's sum + half 1's
                        red[wave][16 * j + (lane & 15)] = ss[j][lane] + ss[j][lane ^ 16]
            for c in range(64):
                part[r, 64 * ct + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c]
    return part


def test_order_model_against_a_lane_by_lane_replay():
    NP, M = 192, 64                                                   # two chunks, the second with two waves without rows
    A, B = _random_operands(NP, M, 77)
    e = np.random.RandomState(78).randint(-30, 31, size=NP)
    L = R.level_sums(A, B)
    wscale = R.scale_of_exponent(e)
    model = R.order_model_part(L, wscale)
    replay = _lane_replay(L, wscale, NP, M)
    assert model.shape == (2, 64) and np.array_equal(model, replay)
    assert np.all(model > 0)
    # and it is a sum of squares of the exact v to the stated bound
    units = R.part_error_units(model, R.exact_part(L, e))
    assert units <= R.PART_BOUND_UNITS, units
    # a plain (unfused, another order) sum differs in some bit: the model's order is not vacuous
    v = R.combine(L) * wscale[:, None]
    plain = np.stack([(v[:128] ** 2).sum(0), (v[128:] ** 2).sum(0)])
    assert not np.array_equal(plain, model)


def test_fma_primitive_is_fused():
    a = np.array([1.0 + 2.0 ** -30, 3.0, 1e-200])
    s = np.array([-1.0, 1.0, 0.0])
    got = R.fma_sq(a, s)
    assert list(got) == [_fma(x, x, y) for x, y in zip(a, s)]
    assert got[0] != a[0] * a[0] + s[0]                              # the product's low bits survive only when fused
