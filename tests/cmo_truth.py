"""Test infrastructure for the constrained multi-objective calls (gpmo_cehvi_argbest, gpmo_cnhvi_greedy; never imported by the
product): the rules of include/gpmo.h restated in NumPy from the truths of the calls they compose — ehvi_truth (the EHVI),
log_cei_truth (the log feasibility), scbo_truth / cnei_truth (the violation fold and the mask), qnehvi_truth (fronts, strips, greedy).

    cehvi:  E = ehvi_values;  s = sum_j log p_j, j ascending from 0;  key = -(E exp(s))  |  -(log E + s)
    cnhvi:  values (2 + C, T, n): slots 0, 1 the objectives' draws, slot 2 + j constraint j's;  viol as gpbo_cnei_greedy's over the
            constraints in slot order;  g0 = masked(f0, viol);  objective 1 raw;  then qnehvi_truth's fronts and greedy on (g0, f1);
            feasible[j] = the share of draws with g0_t(pick_j) > -inf, NaN for a NaN pick."""
import numpy as np

import cnei_truth as CT
import ehvi_truth as ET
import log_cei_truth as LC
import qnehvi_truth as QT
import scbo_truth as ST


def log_feasibility(cm, cs, lb, ub):
    """s (M,) from the constraints' posteriors cm, cs (C, M) and bounds (C,): log_cei_truth's restatement of the header, j ascending
    into one accumulator from 0"""
    cm, cs = np.atleast_2d(np.asarray(cm, dtype=np.float64)), np.atleast_2d(np.asarray(cs, dtype=np.float64))
    s = np.zeros(cm.shape[1])
    with np.errstate(all="ignore"):
        for j in range(cm.shape[0]):
            s = s + np.array([LC._log_p(lb[j], ub[j], cm[j, i], cs[j, i])[0] for i in range(cm.shape[1])])
    return s


def cehvi_keys(mu, sd, levels, boxes, lb, ub, log_form, product_slip=False):
    """The key (M,) from mu, sd (m + C, M) — the objectives' rows first —, the level rows, boxes = (cell_lo, cell_hi) and the bounds
    (C,).  product_slip: the slip "s added in product form", -(E + exp(s)) / -(log E * s) is not it; the slip is -(log E + exp(s))."""
    m = len(levels)
    mu, sd = np.asarray(mu, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    E = ET.ehvi_values(mu[:m], sd[:m], levels, boxes[0], boxes[1])
    s = log_feasibility(mu[m:], sd[m:], lb, ub)
    with np.errstate(all="ignore"):
        if product_slip:
            return -(np.log(E) + np.exp(s))
        return -(np.log(E) + s) if log_form else -(E * np.exp(s))


def violations(values, lb, ub, y_std, swap=False):
    """viol (T, n) of values (2 + C, T, n): the constraints are slots 2 ..  swap: the slip that takes the constraints' y_std in the
    reverse order (a two-term sum commutes, so a swap of the TERMS changes no bit; a swap of the divisors does, wherever a term is
    not 0 — the mask, which only asks viol == 0, cannot see it: viol_out does)"""
    values = np.asarray(values, dtype=np.float64)
    stds = list(y_std[2:values.shape[0]])
    if swap:
        stds = stds[::-1]
    return ST.violations(values[[0] + list(range(2, values.shape[0]))], lb, ub, [1.0] + stds)


def masked_draws(values, lb, ub, y_std, mask_objective=0, swap=False):
    """((2, T, n) what the score kernel streams, viol (T, n)); mask_objective = 1 is the slip that masks the wrong objective"""
    values = np.asarray(values, dtype=np.float64)
    viol = violations(values, lb, ub, y_std, swap)
    out = np.array(values[:2])
    out[mask_objective] = CT.masked(values[mask_objective], viol)
    return out, viol


def rule(values, base_values, lb, ub, y_std, ref, q, index_offset=0, mask_objective=0, mask_base=True, swap=False):
    """The whole call on given RAW values (2 + C, T, M) and base values (2 + C, T, B): a dict like the engine's, the fronts as lists"""
    g, viol = masked_draws(values, lb, ub, y_std, mask_objective, swap)
    T = g.shape[1]
    if base_values is None or np.shape(base_values)[2] == 0:
        gb = np.empty((2, T, 0))
    elif mask_base:
        gb = masked_draws(base_values, lb, ub, y_std, mask_objective, swap)[0]
    else:
        gb = np.asarray(base_values, dtype=np.float64)[:2]
    return replay(g, gb, ref, q, index_offset, viol)


def replay(g, gb, ref, q, index_offset=0, viol=None):
    """The greedy replay on masked values g (2, T, M) and masked base values gb (2, T, B), with `feasible`"""
    ref = np.asarray(ref, dtype=np.float64)
    f0 = QT.fronts_of(gb, ref) if gb.shape[2] else [np.empty((0, 2)) for _ in range(g.shape[1])]
    idx, gain, keys, f1 = QT.greedy(g, f0, ref, q, index_offset)
    return {"index": idx, "gain": gain, "feasible": CT.pick_feasible(g[0], idx - index_offset, gain), "keys": keys, "viol": viol,
            "fronts_before": f0, "fronts_after": f1, "masked": g, "masked_base": gb}
