"""Test infrastructure for greedy batch noisy expected improvement (gpbo_qnei_greedy / suggest_qnei; never imported by the product):
the greedy of include/gpbo.h restated in NumPy exactly as the header words it, the draws' values from tests/paths_truth.py, and
QneiFakeEngine.

With T draws f_t (rows of `values` (T, M) over the candidates), incumbents m_t (`baseline` (T,)) and steps j = 0 .. q - 1:
    term_t(x) = f_t(x) - m_t  where that is > 0;  0 where it is <= 0;  NaN where f_t(x) is NaN
    key_j(x)  = -((term_0 + term_1 + ... + term_{T-1}) / T)      a sequential loop over t from 0, ONE division;
                +inf for a candidate picked in an earlier step
    pick_j    = the first NaN of key_j, else the first index of its minimum;  gain_j = -key_j there (NaN for a NaN pick)
    m_t       = fmax(m_t, f_t(pick_j))                           a NaN value leaves m_t as it is
`greedy` runs on whatever values it is given — the truth's, or the device's own values_out / baseline_out, whose keys it must then
reproduce bit for bit (no product enters a key, so NumPy's adds and its one division are the device's)."""
import numpy as np

import paths_truth as P


def baseline(train_values, pending_values=None, noisy=True, y_best=None):
    """m_t (T,) before the first pick: the fmax fold, in index order, of the draw's values at the training points (noisy) or of
    y_best, then of its values at the pending points.  train_values (T, N), pending_values (T, P) or None."""
    train_values = np.asarray(train_values, dtype=np.float64)
    T = train_values.shape[0]
    m = np.full(T, np.nan) if noisy else np.full(T, float(y_best))
    cols = [train_values[:, i] for i in range(train_values.shape[1])] if noisy else []
    if pending_values is not None:
        pending_values = np.asarray(pending_values, dtype=np.float64).reshape(T, -1)
        cols += [pending_values[:, i] for i in range(pending_values.shape[1])]
    for col in cols:
        m = np.fmax(m, col)
    return m


def keys_of(values, m, picked):
    """key_j (M,) from the values (T, M), the incumbents (T,) and the picked mask (M,) bool"""
    values = np.asarray(values, dtype=np.float64)
    T, M = values.shape
    total = np.zeros(M)
    with np.errstate(invalid="ignore"):
        for t in range(T):                                     # the order of the sum: t = 0 .. T - 1 into one accumulator from 0
            f = values[t]
            d = f - m[t]
            total = total + np.where(d > 0, d, np.where(np.isnan(f), f, 0.0))
        key = -(total / float(T))                              # one true division
    return np.where(picked, np.inf, key)


def pick_of(key):
    """(index, gain): the first NaN wins (gain NaN), else the first index of the minimum (-0.0 == 0.0; gain = -key there)"""
    nan = np.isnan(key)
    if nan.any():
        return int(np.argmax(nan)), np.nan
    i = int(np.argmin(key))
    return i, -key[i]


def greedy(values, m0, q, index_offset=0):
    """(pick_idx (q,) int64, pick_gain (q,), keys (q, M), m (T,) after the last pick)"""
    values = np.asarray(values, dtype=np.float64)
    T, M = values.shape
    m = np.array(m0, dtype=np.float64)
    picked = np.zeros(M, dtype=bool)
    idx, gain, keys = np.empty(q, dtype=np.int64), np.empty(q), np.empty((q, M))
    for j in range(q):
        keys[j] = keys_of(values, m, picked)
        i, g = pick_of(keys[j])
        idx[j], gain[j] = i + index_offset, g
        picked[i] = True
        m = np.fmax(m, values[:, i])
    return idx, gain, keys, m


def step_gaps(keys):
    """per step: second smallest - smallest key among the unmasked candidates, as a raw difference (the caller divides by the
    range of the values); a step with one unmasked candidate has gap inf"""
    out = []
    for key in np.asarray(keys, dtype=np.float64):
        live = np.sort(key[np.isfinite(key)])
        out.append(np.inf if live.shape[0] < 2 else float(live[1] - live[0]))
    return np.array(out)


def leading_separated_steps(values, keys, floor):
    """How many leading steps have their best and second-best key at least `floor` x (the range of the values) apart."""
    values = np.asarray(values, dtype=np.float64)
    span = float(np.nanmax(values) - np.nanmin(values))
    gaps = step_gaps(keys) / (span if span > 0 else 1.0)
    n = 0
    while n < gaps.shape[0] and gaps[n] >= floor:
        n += 1
    return n, gaps


def group_values(route, kind, X, y_norm, length_scale, eta, groups, points, y_mean=0.0, y_std=1.0, amplitude=1.0):
    """(T, n): the draws of every group — a list of (omega, phase, weights, eps) — at `points`, by paths_truth's `route`
    (P.paths_cho / P.paths_winv / P.paths_mp), rows in group order"""
    return np.vstack([route(kind, X, y_norm, length_scale, eta, om, ph, w, eps, points, y_mean, y_std, amplitude=amplitude)
                      for om, ph, w, eps in groups])


class QneiFakeEngine(P.PathsFakeEngine):
    """paths_truth.PathsFakeEngine (TEST DOUBLE ONLY) + qnei_greedy by `paths_cho` and `greedy` for a unit model."""

    def qnei_greedy(self, groups, q, noisy=True, y_best=0.0, pending=None, slot=0, y_mean=0.0, y_std=1.0, index_offset=0,
                    return_values=False, return_keys=False):
        groups = list(groups)
        shapes = [(np.shape(g[2])[0], np.shape(g[0])[0]) for g in groups]
        self.calls.append(("qnei_greedy", slot, len(groups), shapes[0][0], int(q)))
        if not 1 <= len(groups) <= 16 or len(set(shapes)) != 1 or not 1 <= shapes[0][0] <= 16:
            raise ValueError("qnei_greedy: bad groups")
        X, kernel, length_scale, noise = self.inputs[slot]
        yn = self.targets[slot]
        if not 1 <= q <= min(64, self.Xc.shape[0]):
            raise ValueError("qnei_greedy: q out of range")
        self.qnei_args = {"noisy": bool(noisy), "y_best": float(y_best), "pending": None if pending is None else np.array(pending),
                          "y_mean": y_mean, "y_std": y_std, "groups": groups}
        vals = group_values(P.paths_cho, kernel, X, yn, length_scale, noise, groups, self.Xc, y_mean, y_std)
        at_train = group_values(P.paths_cho, kernel, X, yn, length_scale, noise, groups, X, y_mean, y_std)
        at_pending = None
        if pending is not None:
            at_pending = group_values(P.paths_cho, kernel, X, yn, length_scale, noise, groups, np.asarray(pending), y_mean, y_std)
        m0 = baseline(at_train, at_pending, noisy, y_best)
        idx, gain, keys, _ = greedy(vals, m0, int(q), index_offset)
        self.qnei_values, self.qnei_baseline = vals, m0
        return idx, gain, m0, (vals if return_values else None), (keys if return_keys else None)
