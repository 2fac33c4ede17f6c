"""Test infrastructure for constrained Thompson sampling (gpbo_sample_paths_constrained / suggest_constrained_thompson /
suggest_scbo; never imported by the product): the rule of include/gpbo.h restated in NumPy over GIVEN value arrays, and
ScboFakeEngine.

values (1 + C, S, M): slot 0 the objective's draws, slot j constraint j's.  Per path s and candidate x
    t_j       = max(max(lb_j - c_j, c_j - ub_j), 0) / y_std_j
    viol_s(x) = t_1 + ... + t_C, added in that order; a NaN c_j makes it NaN
and the pick per path: the first NaN (of f_s or viol_s) wins; else the first index of the largest f_s among viol_s == 0; else the
first index of the least viol_s."""
import numpy as np

import paths_truth as P
import turbo_truth as T


def violations(values, lb, ub, y_std):
    """viol (S, M) of values (1 + C, S, M); y_std (1 + C,) — entry 0, the objective's, is not used"""
    values = np.asarray(values, dtype=np.float64)
    total = None
    with np.errstate(invalid="ignore"):
        for j in range(1, values.shape[0]):
            c = values[j]
            t = np.maximum(np.maximum(lb[j - 1] - c, c - ub[j - 1]), 0.0) / y_std[j]      # np.maximum propagates NaN
            total = t if total is None else total + t
    return total


def picks(f, viol, index_offset=0):
    """(idx (S,), val (S,), best_viol (S,), feasible (S,) bool) from the objective's values f (S, M) and viol (S, M)"""
    f, viol = np.asarray(f, dtype=np.float64), np.asarray(viol, dtype=np.float64)
    S = f.shape[0]
    idx, val, bv, feas = np.empty(S, dtype=np.int64), np.empty(S), np.empty(S), np.zeros(S, dtype=bool)
    for s in range(S):
        nan = np.isnan(f[s]) | np.isnan(viol[s])
        ok = viol[s] == 0.0
        if nan.any():
            idx[s], val[s], bv[s] = np.flatnonzero(nan)[0], np.nan, np.nan
        elif ok.any():
            idx[s] = int(np.argmax(np.where(ok, f[s], -np.inf)))
            val[s], bv[s], feas[s] = f[s, idx[s]], 0.0, True
        else:
            idx[s] = int(np.argmin(viol[s]))
            val[s], bv[s] = f[s, idx[s]], viol[s, idx[s]]
    return idx + index_offset, val, bv, feas


def rule(values, lb, ub, y_std, index_offset=0):
    viol = violations(values, lb, ub, y_std)
    return picks(np.asarray(values)[0], viol, index_offset) + (viol,)


class ScboFakeEngine(P.PathsFakeEngine):
    """paths_truth.PathsFakeEngine (TEST DOUBLE ONLY) + sample_paths_constrained = `paths_cho` per slot and the rule above, and
    generate_candidates_trust_region by tests/turbo_truth.py; records what it was handed."""

    def sample_paths_constrained(self, draws, lb, ub, y_mean, y_std, index_offset=0, return_values=False):
        draws = list(draws)
        self.calls.append(("sample_paths_constrained", len(draws) - 1, np.shape(draws[0][2])[0]))
        self.constrained_args = getattr(self, "constrained_args", []) + [
            dict(draws=[tuple(np.array(a) for a in t) for t in draws], lb=np.array(lb), ub=np.array(ub), y_mean=np.array(y_mean),
                 y_std=np.array(y_std))]
        vals = []
        for j, (omega, phase, weights, eps) in enumerate(draws):
            X, kernel, length_scale, noise = self.inputs[j]
            vals.append(P.paths_cho(kernel, X, self.targets[j], length_scale, noise, omega, phase, weights, eps, self.Xc, y_mean[j],
                                    y_std[j]))
        vals = np.array(vals)
        idx, val, bv, feas, viol = rule(vals, lb, ub, y_std, index_offset)
        self.constrained_values = getattr(self, "constrained_values", []) + [vals]
        return idx, val, bv, feas, (vals if return_values else None), (viol if return_values else None)

    def generate_candidates_trust_region(self, M, centre, lo, hi, sv, shift, bits, mask_threshold, mask_key):
        self.calls.append(("generate_candidates_trust_region", M))
        self.tr_args = dict(M=M, centre=np.array(centre), lo=np.array(lo), hi=np.array(hi), sv=sv, shift=shift, bits=bits,
                            threshold=mask_threshold, key=mask_key)
        self.Xc = T.generate(M, centre, lo, hi, sv, shift, mask_threshold, mask_key)
        self.n_candidates = M
        self.post = {}
