"""Test infrastructure for the nearest-neighbour GP scoring (gpnn_acq_argbest / suggest_local; never imported by the product): a plain
reference of include/gpnn.h's formulas from X, y, theta and the candidates alone.  The neighbours come from a stable sort on (d2,
index), d2 in fp64 by the header's ascending-t sum (a multiply and an add per term, where the device has one fma); the local solves
and acquisition values run in `dtype` (np.longdouble, or np.float64 for the reference's own spread), batched over the candidates."""
import mpmath as mp
import numpy as np
from scipy import special

import matern_family_truth as F

UCB, EI, POI, LOG_EI = 0, 1, 2, 3


def neighbours(X, ls, Xc, k):
    """(indices (M, k), nearest first, ties to the lower index; the smallest relative gap of the k-th and (k + 1)-th d2, inf at N == k)"""
    Xs, Ps = np.asarray(X, dtype=np.float64) / ls, np.asarray(Xc, dtype=np.float64) / ls
    d2 = np.zeros((Ps.shape[0], Xs.shape[0]))
    for t in range(Xs.shape[1]):
        df = Ps[:, t, None] - Xs[None, :, t]
        d2 = d2 + df * df
    if Xs.shape[0] > 4096:      # a full sort of every row is slow: the k + 1 smallest first (exact unless the returned gap is 0)
        part = np.sort(np.argpartition(d2, k, axis=1)[:, :k + 1], axis=1)
        sub = np.take_along_axis(d2, part, axis=1)
        order = np.take_along_axis(part, np.argsort(sub, axis=1, kind="stable"), axis=1)
    else:
        order = np.argsort(d2, axis=1, kind="stable")
    if Xs.shape[0] == k:
        return order, np.inf
    srt = np.take_along_axis(d2, order, axis=1)
    return order[:, :k], float(((srt[:, k] - srt[:, k - 1]) / srt[:, k]).min())


def posterior(kind, X, yn, ls, alpha, Xc, nbr, y_mean, y_std, c=1.0, w=0.0, dtype=np.longdouble):
    """(mu (M,), sd (M,)) in `dtype`: per candidate the GP c k + (c w + alpha) I conditioned on its rows `nbr` (M, k)"""
    ls = np.asarray(ls, dtype=dtype)
    Xn = np.asarray(X, dtype=dtype)[nbr] / ls                      # (M, k, d)
    P = np.asarray(Xc, dtype=dtype) / ls
    k = nbr.shape[1]
    A = dtype(c) * F.kernel_value(kind, np.sqrt(((Xn[:, :, None, :] - Xn[:, None, :, :]) ** 2).sum(-1)))
    A[:, np.arange(k), np.arange(k)] = dtype(c) + (dtype(c) * dtype(w) + dtype(alpha))
    v = dtype(c) * F.kernel_value(kind, np.sqrt(((Xn - P[:, None, :]) ** 2).sum(-1)))      # (M, k): k*
    u = np.asarray(yn, dtype=dtype)[nbr].copy()
    for j in range(k):      # right-looking Cholesky with both right-hand sides in the sweep
        ljj = np.sqrt(A[:, j, j])
        col = A[:, j + 1:, j] / ljj[:, None]
        u[:, j], v[:, j] = u[:, j] / ljj, v[:, j] / ljj
        u[:, j + 1:] -= col * u[:, j, None]
        v[:, j + 1:] -= col * v[:, j, None]
        A[:, j + 1:, j + 1:] -= col[:, :, None] * col[:, None, :]
    mu = dtype(y_mean) + dtype(y_std) * (v * u).sum(1)
    return mu, dtype(y_std) * np.sqrt(np.maximum(dtype(c) - (v * v).sum(1), 0))


def neg_acquisition(acq, mu, sd, param, y_max):
    """-acq(mu, sd) in mu's dtype; Phi and phi through SciPy's fp64 (their rounding is 1e-16 of the value)"""
    dtype = mu.dtype.type
    if acq == UCB:
        return -(mu + dtype(param) * sd)
    aa = mu - dtype(y_max) - dtype(param)
    if acq == LOG_EI:      # log(sd) + log(phi(z) + z Phi(z)), the second term at 50 digits: the sum cancels in the lower tail
        with mp.workdps(50):
            logh = []
            for z in aa / sd:
                zz = mp.mpf(float(z)) + mp.mpf(float(z - dtype(float(z))))
                v = mp.log(mp.npdf(zz) + zz * mp.ncdf(zz))
                logh.append(dtype(float(v)) + dtype(float(v - mp.mpf(float(v)))))
        return -(np.log(sd) + np.array(logh, dtype=dtype))
    z = (aa / sd).astype(np.float64)
    cdf, pdf = special.ndtr(z).astype(dtype), (np.exp(-z * z / 2) / np.sqrt(2 * np.pi)).astype(dtype)
    return -cdf if acq == POI else -(aa * cdf + sd * pdf)


def nngp(kind, X, yn, ls, alpha, Xc, k, acq, param, y_max, y_mean, y_std, c=1.0, w=0.0):
    """One call's reference in longdouble, and "D": its largest distance from the same in fp64 over the same sets, per 1 + |value|"""
    nbr, gap = neighbours(X, ls, Xc, k)
    out = {}
    for dtype in (np.longdouble, np.float64):
        mu, sd = posterior(kind, X, yn, ls, alpha, Xc, nbr, y_mean, y_std, c, w, dtype)
        out[dtype] = (mu, sd, neg_acquisition(acq, mu, sd, param, y_max))
    hi, lo = out[np.longdouble], out[np.float64]
    D = max(float((np.abs(h - l) / (1 + np.abs(h))).max()) for h, l in zip(hi, lo))
    return {"nbr": nbr, "gap": gap, "mu": hi[0], "sd": hi[1], "ys": hi[2], "D": D}
