"""include/gppf.h restated: `pfes` in plain fp64 NumPy with the header's tail-side differences and conventions; `pfes_ext`, the same
quantity from mpmath at 30 digits by the textbook form (differences of Phi) for ONE candidate — used only to size `pfes`' own
noise —; and `staircase`, the front of a set of value pairs by gpbo_qnhvi_greedy's rule without a reference point."""
import mpmath
import numpy as np
from scipy.special import erfc

TINY = np.finfo(np.float64).tiny


def level(lv, mu, sd):
    """(L, U, psi, z >= 0) of the level `lv` for every candidate"""
    with np.errstate(all="ignore"):
        z = (lv - mu) / sd
        t = erfc(np.abs(z) / np.sqrt(2.0)) / 2.0
        up = z >= 0
        pdf = np.exp(-(z * z) / 2.0) / np.sqrt(2.0 * np.pi)
        L, psi = np.where(up, 1.0 - t, t), np.where(pdf == 0.0, 0.0, z * pdf)
    step = sd == 0
    L = np.where(step, (lv >= mu) * 1.0, L)
    return L, np.where(step, 1.0 - L, np.where(up, t, 1.0 - t)), np.where(step, 0.0, psi), up


def pfes(mu0, sd0, mu1, sd1, fronts, sizes):
    """(a (M,) in nats, the smallest Z_s of each candidate (M,)); fronts (S, 128, 2), sizes (S,)"""
    M, S = len(mu0), len(sizes)
    acc, zmin = np.zeros(M), np.full(M, np.inf)
    for s in range(S):
        f, n = fronts[s], int(sizes[s])
        Z, Q = np.zeros(M), np.zeros(M)
        Lk, Uk, pk, _ = level(f[0, 0], mu0, sd0)
        for k in range(n):
            Ln, Un, pn, upn = level(f[k + 1, 0], mu0, sd0) if k + 1 < n else (np.zeros(M), np.ones(M), np.zeros(M), np.zeros(M, bool))
            L1, _, p1, _ = level(f[k, 1], mu1, sd1)
            P0 = np.where(upn, Un - Uk, Lk - Ln)
            Z = Z + P0 * L1
            Q = Q + ((pn - pk) * L1 + P0 * (-p1))
            Lk, Uk, pk = Ln, Un, pn
        with np.errstate(all="ignore"):
            acc = acc + np.where(Z < TINY, 0.0, -np.log(Z) - Q / (2.0 * Z))
        zmin = np.minimum(zmin, Z)
    return np.where(np.isnan(mu0) | np.isnan(sd0) | np.isnan(mu1) | np.isnan(sd1), np.nan, acc / S), zmin


def pfes_ext(mu0, sd0, mu1, sd1, fronts, sizes):
    """a of ONE candidate (sd > 0) at 30 digits: Z = sum (Phi(u0) - Phi(l0)) Phi(u1), Q from l phi(l) - u phi(u)"""
    with mpmath.workdps(30):
        psi = lambda z: z * mpmath.npdf(z)      # noqa: E731
        acc = mpmath.mpf(0)
        for s in range(len(sizes)):
            n, Z, Q = int(sizes[s]), mpmath.mpf(0), mpmath.mpf(0)
            u0 = (mpmath.mpf(fronts[s, 0, 0]) - mu0) / sd0
            cu, pu = mpmath.ncdf(u0), psi(u0)
            for k in range(n):
                u1 = (mpmath.mpf(fronts[s, k, 1]) - mu1) / sd1
                l0 = (mpmath.mpf(fronts[s, k + 1, 0]) - mu0) / sd0 if k + 1 < n else None
                cl, pl = (mpmath.ncdf(l0), psi(l0)) if k + 1 < n else (0, 0)
                c1 = mpmath.ncdf(u1)
                Z += (cu - cl) * c1
                Q += (pl - pu) * c1 - (cu - cl) * psi(u1)
                cu, pu = cl, pl
            acc += 0 if Z < TINY else -mpmath.log(Z) - Q / (2 * Z)
        return float(acc / len(sizes))


def staircase(v0, v1):
    """The front (n, 2) of the pairs without a NaN: objective 0 descending, objective 1 strictly ascending; equal pairs count once"""
    ok = ~(np.isnan(v0) | np.isnan(v1))
    a, c = v0[ok], v1[ok]
    pts, floor = [], -np.inf
    for i in np.lexsort((-c, -a)):
        if c[i] > floor:
            pts.append((a[i], c[i]))
            floor = c[i]
    return np.array(pts).reshape(-1, 2)
