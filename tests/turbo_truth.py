"""Test infrastructure for the trust-region candidate generator (gpbo_generate_candidates_trust_region / suggest_turbo; never
imported by the product): a NumPy restatement of the definition in include/gpbo.h — Philox4x32-10, the closed-form points of a
scrambled Sobol sequence, the perturbation mask with its fallback column, and the assembly of the matrix.  Everything is integer
arithmetic up to  lo + (hi - lo) * u  with u = w 2^-bits exact, so the device is compared BIT FOR BIT.  tests/test_turbo_host.py
checks this file against SciPy's own Sobol engine before tests/test_gpu_turbo.py lets it judge the device.
"""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, key: int):
    """Four uint32 arrays: Philox4x32-10 (Salmon et al. 2011) of the counters (c0, c1, c2, c3), each an array of one shape, under
    the 64-bit `key` (low word k0, high word k1).  Known answer (Random123 kat_vectors): counter 0, key 0 -> 6627e8d5 e169c58d
    bc57ac4c 9b00dbd8."""
    c = [np.asarray(v, dtype=np.uint64) & _LOW for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]             # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _LOW, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _LOW]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def sobol_words(M: int, sv, shift) -> np.ndarray:
    """(M, d) uint32: w(m, t) = shift[t] XOR over the set bits b of g = m ^ (m >> 1) of sv[t, b]."""
    sv, shift = np.asarray(sv, dtype=np.uint32), np.asarray(shift, dtype=np.uint32)
    m = np.arange(int(M), dtype=np.uint64)
    g = m ^ (m >> np.uint64(1))
    w = np.broadcast_to(shift, (int(M), shift.shape[0])).copy()
    for b in range(sv.shape[1]):
        on = ((g >> np.uint64(b)) & np.uint64(1)).astype(bool)
        w[on] ^= sv[:, b]
    assert not (g >> np.uint64(sv.shape[1])).any(), "M exceeds 2^bits"
    return w


def sobol_unit(M: int, sv, shift) -> np.ndarray:
    """(M, d) float64 in [0, 1): u = w 2^-bits, exact."""
    return sobol_words(M, sv, shift).astype(np.float64) * 2.0 ** -int(np.asarray(sv).shape[1])


def mask(M: int, d: int, threshold: int, key: int) -> np.ndarray:
    """(M, d) bool: element e = m d + t is perturbed iff word e & 3 of philox((e >> 2, 0, 0), key) < threshold; a row without a
    perturbed coordinate gets column (w0 d) >> 32, w0 = word 0 of philox((m, 1, 0), key)."""
    M, d = int(M), int(d)
    e = np.arange(M * d, dtype=np.uint64)
    q = e >> np.uint64(2)
    words = np.stack(philox4x32_10(q & _LOW, q >> _S32, 0, 0, key), axis=1)            # (M d, 4)
    word = words[np.arange(M * d), (e & np.uint64(3)).astype(np.int64)]
    out = (word.astype(np.uint64) < np.uint64(int(threshold))).reshape(M, d)
    m = np.arange(M, dtype=np.uint64)
    w0 = philox4x32_10(m & _LOW, m >> _S32, 1, 0, key)[0]
    column = ((w0.astype(np.uint64) * np.uint64(d)) >> _S32).astype(np.int64)
    empty = ~out.any(axis=1)
    out[empty, column[empty]] = True
    return out


def generate(M: int, centre, lo, hi, sv, shift, threshold: int, key: int) -> np.ndarray:
    """The (M, d) matrix gpbo_generate_candidates_trust_region leaves resident."""
    centre, lo, hi = (np.asarray(v, dtype=np.float64) for v in (centre, lo, hi))
    points = lo + (hi - lo) * sobol_unit(M, sv, shift)
    return np.where(mask(M, centre.shape[0], threshold, key), points, centre)
