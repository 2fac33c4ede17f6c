"""Truth for expected hypervolume improvement (tests only; never imported by the product).

    g_j(a)  = E[(Y_j - a)^+] = sd_j f((mu_j - a) / sd_j),   f(z) = phi(z) + z Phi(z),   g_j(+inf) = 0
    EHVI(x) = sum_k prod_j (g_j(l_kj) - g_j(u_kj))

`f_truth` / `ehvi_truth`: f and the cell sum in mpmath at 60 digits, Phi taken from erfc on BOTH sides (at z = -40 the two halves of
f agree to 3 digits and are 1e-348 each; 60 digits carry that).  `ehvi_truth` also returns the magnitude sum S.
`ehvi_values`: the two-range form of include/gpbo.h in NumPy / SciPy with the conventions (sd == 0 -> (mu - a)^+, NaN propagates), and
the magnitude sum S(x) = sum_k prod_j (g_j(l) + g_j(u)): what the cells' cancellation is measured against.
`hvi_brute`: the hypervolume improvement of a point over a front by counting the cells of the coordinate grid — no box decomposition,
no level lists, nothing of bayesianoptimization_amd/multiobjective.py.
`argbest`: numpy's argmin / min / stable argsort[:k] over a key, as gpbo_acq_argbest states them.
"""
import mpmath
import numpy as np
from scipy import special

_ctx = mpmath.mp.clone()
_ctx.dps = 60

BAR = 1e-9             # the project's bar on a value, relative ...
FLOOR = 1e-4           # ... to max(|truth|, FLOOR * S): where cells cancel, S is what the rounding scales with
TINY = 1e-290          # ... and values below this are held to BAR * TINY absolutely
SERIES_BELOW = -28.0   # csrc/acq_formulas.h: LOG_EI_SERIES_BELOW


# ---- 60 digits ---------------------------------------------------------------------------------------------------------------------
def f_truth(z):
    """f(z) = phi(z) + z Phi(z) as an mpmath number; z an mpmath number or a float"""
    c = _ctx
    z = c.mpf(z)
    phi = c.exp(-z * z / 2) / c.sqrt(2 * c.pi)
    cdf = 1 - c.erfc(z / c.sqrt(2)) / 2 if z > 0 else c.erfc(-z / c.sqrt(2)) / 2
    return phi + z * cdf


def z_mp(mu, sd, a):
    """(mu - a) / sd of three floats, formed in 60 digits"""
    return (_ctx.mpf(float(mu)) - _ctx.mpf(float(a))) / _ctx.mpf(float(sd))


def g_truth(mu, sd, a):
    c = _ctx
    if np.isposinf(a):
        return c.mpf(0)
    if sd == 0.0:
        return max(c.mpf(float(mu)) - c.mpf(float(a)), c.mpf(0))
    return c.mpf(float(sd)) * f_truth(z_mp(mu, sd, a))


def ehvi_truth(mu, sd, levels, cell_lo, cell_hi):
    """(EHVI, S) of ONE candidate as floats rounded from 60 digits: mu, sd (m,); levels m rows; cell_lo / cell_hi (K, m)"""
    m = len(levels)
    tables = [[g_truth(mu[j], sd[j], a) for a in np.asarray(levels[j], dtype=np.float64)] for j in range(m)]
    total, scale = _ctx.mpf(0), _ctx.mpf(0)
    for lo, hi in zip(np.asarray(cell_lo), np.asarray(cell_hi)):
        p, q = _ctx.mpf(1), _ctx.mpf(1)
        for j in range(m):
            p *= tables[j][lo[j]] - tables[j][hi[j]]
            q *= tables[j][lo[j]] + tables[j][hi[j]]
        total += p
        scale += q
    return float(total), float(scale)


# ---- fp64 --------------------------------------------------------------------------------------------------------------------------
def _ratio(z):
    """r = 1 + z Phi(z) / phi(z) for z <= -1: erfcx down to SERIES_BELOW, ten terms of the asymptotic series below it"""
    r = np.empty_like(z)
    near = z > SERIES_BELOW
    t = -z[near] * 0.70710678118654752440
    r[near] = 1.0 - 1.77245385090551602730 * t * special.erfcx(t)
    w = 1.0 / (z[~near] * z[~near])
    s = np.full_like(w, -654729075.0)
    for c in (34459425.0, -2027025.0, 135135.0, -10395.0, 945.0, -105.0, 15.0, -3.0, 1.0):
        s = s * w + c
    r[~near] = w * s
    return r


def f_values(z):
    """f over an array by the two-range form: as written above -1, phi(z) r(z) from -1 down, 0 where phi underflows"""
    z = np.asarray(z, dtype=np.float64)
    out = np.full(z.shape, np.nan)
    with np.errstate(all="ignore"):
        up = z > -1.0
        out[up] = np.exp(-(z[up] * z[up]) / 2.0) / 2.50662827463100050242 + z[up] * special.ndtr(z[up])
        low = z <= -1.0
        phi = np.exp(-(z[low] * z[low]) / 2.0) / 2.50662827463100050242
        out[low] = np.where(phi == 0.0, 0.0, phi * _ratio(z[low]))
    return out


def g_values(mu, sd, a):
    """g (M,) of one level a for mu, sd (M,)"""
    with np.errstate(all="ignore"):
        if np.isposinf(a):
            g = np.zeros(mu.shape)
        else:
            g = np.where(sd == 0.0, np.maximum(mu - a, 0.0), sd * f_values((mu - a) / np.where(sd == 0.0, 1.0, sd)))
    return g


def ehvi_values(mu, sd, levels, cell_lo, cell_hi, return_scale=False):
    """EHVI (M,) >= 0 from mu, sd (m, M), the level rows and the cells (K, m); with return_scale also S (M,).  A NaN mu or sd in any
    objective -> NaN."""
    mu, sd = np.atleast_2d(np.asarray(mu, dtype=np.float64)), np.atleast_2d(np.asarray(sd, dtype=np.float64))
    cell_lo, cell_hi = np.asarray(cell_lo), np.asarray(cell_hi)
    m = len(levels)
    value, scale = None, None
    for j in range(m):
        table = np.stack([g_values(mu[j], sd[j], a) for a in np.asarray(levels[j], dtype=np.float64)])      # (L_j, M)
        lo, hi = table[cell_lo[:, j]], table[cell_hi[:, j]]
        value = lo - hi if value is None else value * (lo - hi)
        if return_scale:
            scale = lo + hi if scale is None else scale * (lo + hi)
    nan = np.isnan(mu).any(axis=0) | np.isnan(sd).any(axis=0)
    out = np.where(nan, np.nan, value.sum(axis=0))
    if return_scale:
        return out, np.where(nan, np.nan, scale.sum(axis=0))
    return out


def trim(n_levels, levels):
    """the level rows of `box_decomposition` without their padding"""
    return [np.asarray(levels[j][:n_levels[j]], dtype=np.float64) for j in range(len(n_levels))]


def bound(truth, scale):
    """the bar on |device - truth|, elementwise"""
    return BAR * np.maximum(np.maximum(np.abs(truth), FLOOR * np.abs(scale)), TINY)


def within_bar(got, truth, scale):
    """(worst |got - truth| / bound, ok); NaNs must sit at the same places"""
    got, truth, scale = (np.asarray(v, dtype=np.float64) for v in (got, truth, scale))
    if not np.array_equal(np.isnan(got), np.isnan(truth)):
        return np.inf, False
    fin = ~np.isnan(truth)
    ratio = np.abs(got[fin] - truth[fin]) / bound(truth[fin], scale[fin])
    worst = float(ratio.max()) if ratio.size else 0.0
    return worst, worst <= 1.0


# ---- brute force -------------------------------------------------------------------------------------------------------------------
def _dominated_volume(P, ref, top):
    """Volume of the part of the box [ref, top) that the rows of P dominate (z is dominated by p when z <= p everywhere): the cells
    of the grid over every coordinate that occurs, each either inside or outside."""
    m = ref.shape[0]
    if np.any(top <= ref):
        return 0.0
    P = np.minimum(P[np.all(P > ref, axis=1)], top)
    if P.shape[0] == 0:
        return 0.0
    edges = [np.unique(np.concatenate([[ref[j]], P[:, j], [top[j]]])) for j in range(m)]
    upper = [e[1:] for e in edges]
    inside = np.zeros([u.shape[0] for u in upper], dtype=bool)
    for p in P:
        mask = upper[0] <= p[0]
        for j in range(1, m):
            mask = np.multiply.outer(mask, upper[j] <= p[j])
        inside |= mask.astype(bool)
    vol = np.diff(edges[0])
    for j in range(1, m):
        vol = np.multiply.outer(vol, np.diff(edges[j]))
    return float(vol[inside].sum())


def hv_brute(Y, ref):
    Y, ref = np.atleast_2d(np.asarray(Y, dtype=np.float64)), np.asarray(ref, dtype=np.float64)
    if Y.size == 0:
        return 0.0
    return _dominated_volume(Y, ref, np.maximum(Y.max(axis=0), ref) + 1.0)


def hvi_brute(front, ref, y):
    """Hypervolume improvement of the point y (m,) over the rows of `front` above `ref`: the volume of [ref, y) less its dominated part"""
    front, ref, y = np.asarray(front, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if np.any(y <= ref):
        return 0.0
    front = front.reshape(-1, ref.shape[0])
    return float(np.prod(y - ref)) - _dominated_volume(front, ref, y)


def front_brute(Y, ref):
    """rows strictly above ref and not dominated, duplicates once, first appearance first — by the double loop"""
    Y = np.asarray(Y, dtype=np.float64).reshape(-1, len(ref))
    keep = []
    for i, y in enumerate(Y):
        if not np.all(y > ref):
            continue
        if any(np.all(z >= y) and np.any(z > y) for z in Y):
            continue
        if any(np.array_equal(Y[k], y) for k in keep):
            continue
        keep.append(i)
    return Y[keep]


# ---- selection ---------------------------------------------------------------------------------------------------------------------
def argbest(ys, k=0, index_offset=0):
    """(best_idx, best_val, seed_idx (k,), seed_val (k,)) of the key ys: argmin / min with the first NaN winning; argsort[:k] with
    ties to the lowest index, -0.0 == 0.0 and NaNs last"""
    ys = np.asarray(ys, dtype=np.float64)
    nan = np.isnan(ys)
    if nan.any():
        bi, bv = int(np.flatnonzero(nan)[0]), float("nan")
    else:
        bi, bv = int(ys.argmin()), float(ys.min())
    order = np.lexsort((np.arange(len(ys)), np.where(nan, np.inf, ys) + 0.0, nan))[:k]
    return bi + index_offset, bv, order + index_offset, ys[order]


def separated_top(a, scale, k):
    """True when the k + 1 largest a are pairwise further apart than twice their bars: the top-k ranking is then the same for every
    evaluation within the bar"""
    a, scale = np.asarray(a, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    order = np.argsort(-np.where(np.isnan(a), -np.inf, a), kind="stable")[:k + 1]
    top, b = a[order], bound(a[order], scale[order])
    if top.size < 2:
        return True
    return bool(np.all(top[:-1] - top[1:] > b[:-1] + b[1:]))


# ---- fronts ------------------------------------------------------------------------------------------------------------------------
def random_front(n, m, seed, lo=0.2, hi=1.0):
    """n mutually non-dominated points in (lo, hi)^m with distinct values per objective: on the simplex-like surface sum_j t_j^2 = 1"""
    rs = np.random.RandomState(seed)
    if n == 0:
        return np.empty((0, m))
    if m == 2:
        ang = np.sort(rs.uniform(0.05, 0.5 * np.pi - 0.05, n))
        pts = np.column_stack([np.cos(ang), np.sin(ang)])
    else:
        u = np.abs(rs.standard_normal((n, m))) + 0.05
        pts = u / np.linalg.norm(u, axis=1, keepdims=True)
    return lo + (hi - lo) * pts
