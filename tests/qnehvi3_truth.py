"""Test infrastructure for gpmo3_nhvi_greedy / suggest_qnehvi3 (never imported by the product): the stored order of a front, the
height-map sweep, the cell sum, the update rule and the greedy of include/gpmo3.h restated in NumPy as the header words them: two
rounded products per cell, the terms in emission order, the draws in order, ONE division.  `pick_of` is tests/qnehvi_truth.py's."""
import numpy as np

import paths_truth as P
from bayesianoptimization_amd.multiobjective import pareto_front
from qnehvi_truth import FrontOverflow, pick_of

L = 128           # GPBO_MAX_QNEHVI_FRONT


def stored(front):
    """the rows (n, 3) in the stored order"""
    front = np.asarray(front, dtype=np.float64).reshape(-1, 3)
    return front[np.lexsort((-front[:, 1], -front[:, 0], -front[:, 2]))]


def front_of(triples, ref):
    """The front (n, 3) of the triples (B, 3): distinct, strictly above ref in all three, no NaN, not dominated (`pareto_front`)"""
    triples = np.asarray(triples, dtype=np.float64).reshape(-1, 3)
    triples = triples[~np.isnan(triples).any(axis=1)]
    return stored(pareto_front(triples, ref) if triples.shape[0] else triples)


def fronts_of(base_values, ref):
    """per draw t the front of base_values[:, t, :].T; base_values (3, T, B)"""
    base_values = np.asarray(base_values, dtype=np.float64)
    return [front_of(base_values[:, t].T, ref) for t in range(base_values.shape[1])]


def sweep(front, ref):
    """The cells (n_cells, 5) of a front in stored order, in emission order"""
    S, cells = [], []      # S: the staircase in (x, y), x descending, y strictly ascending
    for a, b, c in np.asarray(front, dtype=np.float64).reshape(-1, 3):
        p = sum(1 for s in S if s[0] > a)
        r = p
        while r < len(S) and S[r][1] <= b:
            r += 1
        for k in range(p, r + 1):
            x_hi = a if k == p else S[k - 1][0]
            x_lo = S[k][0] if k < len(S) else ref[0]
            y_lo = S[k - 1][1] if k > 0 else ref[1]
            if x_hi != x_lo:
                cells.append((x_lo, x_hi, y_lo, b, c))
        S[p:r] = [(a, b)]
    for k in range(len(S) + 1):
        cells.append((S[k][0] if k < len(S) else ref[0], np.inf if k == 0 else S[k - 1][0], S[k - 1][1] if k > 0 else ref[1], np.inf,
                      ref[2]))
    return np.array(cells, dtype=np.float64).reshape(-1, 5)


def hvi(f, cells):
    """HVI of the values f (3, M) against one draw's cells: the terms in emission order into one accumulator from 0"""
    f0, f1, f2 = np.asarray(f, dtype=np.float64)
    total = np.zeros(f0.shape)
    with np.errstate(invalid="ignore"):
        for x_lo, x_hi, y_lo, y_hi, h in cells:
            w, v, u = np.minimum(f0, x_hi) - x_lo, np.minimum(f1, y_hi) - y_lo, f2 - h
            total = total + (np.where(w > 0, w, 0.0) * np.where(v > 0, v, 0.0)) * np.where(u > 0, u, 0.0)
    return np.where(np.isnan(f0) | np.isnan(f1) | np.isnan(f2), np.nan, total)


def keys_of(values, cells, picked):
    """key_j (M,) from the values (3, T, M), the T draws' cells and the picked mask (M,) bool"""
    _, T, M = values.shape
    total = np.zeros(M)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            total = total + hvi(values[:, t], cells[t])
        key = -(total / float(T))
    return np.where(picked, np.inf, key)


def insert(front, y, ref):
    """(the front after it absorbs y (3,), whether it changed)"""
    y = np.asarray(y, dtype=np.float64)
    if np.isnan(y).any() or not (y > np.asarray(ref)).all():
        return front, False
    if front.shape[0] and np.any((front >= y).all(axis=1)):
        return front, False
    out = stored(np.vstack([front[~(front <= y).all(axis=1)], y[None]]))
    if out.shape[0] > L:
        raise FrontOverflow()
    return out, True


def greedy(values, fronts, cells, ref, q, index_offset=0):
    """(pick_idx (q,) int64, pick_gain (q,), keys (q, M), the fronts and the cells after the last pick)"""
    values = np.asarray(values, dtype=np.float64)
    _, T, M = values.shape
    fronts, cells = [np.array(f).reshape(-1, 3) for f in fronts], [np.array(c).reshape(-1, 5) for c in cells]
    picked = np.zeros(M, dtype=bool)
    idx, gain, keys = np.empty(q, dtype=np.int64), np.empty(q), np.empty((q, M))
    for j in range(q):
        keys[j] = keys_of(values, cells, picked)
        i, g = pick_of(keys[j])
        idx[j], gain[j] = i + index_offset, g
        picked[i] = True
        for t in range(T):
            fronts[t], changed = insert(fronts[t], values[:, t, i], ref)
            if changed:
                cells[t] = sweep(fronts[t], ref)
    return idx, gain, keys, fronts, cells


def same_rows(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


class Qnehvi3FakeEngine(P.PathsFakeEngine):
    """paths_truth.PathsFakeEngine (TEST DOUBLE ONLY) + a qnehvi3_greedy that records what it is given and picks 0 .. q - 1"""

    def qnehvi3_greedy(self, draws, q, ref, base=None, y_mean=(0.0,) * 3, y_std=(1.0,) * 3, index_offset=0, return_fronts=False):
        draws = [list(g) for g in draws]
        self.calls.append(("qnehvi3_greedy", len(draws[0]), np.shape(draws[0][0][2])[0], int(q)))
        self.qnehvi3_args = {"ref": np.asarray(ref), "base": np.array(base), "y_mean": list(y_mean), "y_std": list(y_std), "draws": draws}
        T = len(draws[0]) * np.shape(draws[0][0][2])[0]
        return {"index": np.arange(q) + index_offset, "gain": np.linspace(1.0, 0.5, q),
                "front_size": np.array([[3] * T, [4] * T], dtype=np.int32) if return_fronts else None}
