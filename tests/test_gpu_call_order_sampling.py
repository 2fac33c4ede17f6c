"""GPU (-m gpu): the order-of-calls contract (tests/test_gpu_call_order.py: readers are invisible, a slot without a posterior refuses)
for the sampling, batch and Pareto entry points — gpbo_sample_paths, gpbo_sample_paths_constrained, gpbo_ascend_paths,
gpbo_mes_argbest, gpbo_kg_argbest, gpbo_ehvi_argbest, gpbo_qnei_greedy, gpbo_qnhvi_greedy, gpbo_generate_candidates_trust_region —
against EACH OTHER and against gpbo_acq_argbest.  Each of them has a test_reader_only of its own against four older readers at one
shape; suggest_turbo, suggest_qnei, suggest_qnehvi, suggest_kg, suggest_mes, the Pareto optimiser and the constant-liar loop drive
one context with all of them.  The state they share is listed in tests/test_gpu_call_order.py's docstring: ctx->ys ([M] values or
[S][M] negated path values), ctx->Xcs (scaled per call with one slot's length scales), ctx->red (selection records, the generator's
tables, the fit scalars; reallocated when a later call needs more), the pinned selection window, the six workspaces, func_attrs, and
the per-slot posterior with its refreshable state.

Base state: tests/test_gpu_qnehvi.py's case n130+65-m257-f65-d5-3x16-p64 — d = 5, slot 0 N = 130 Matern-1.5 scaled, slot 1 N = 65 RBF
F32 — its draws and base points, over two candidate sets: "A", the case's own M = 257 (odd: one candidate per score thread), and "B",
M = 1024 (even: two; other workspace offsets, another extent of ctx->ys).  No call refused the scaled or the F32 slot, so no further
slot was needed.  CALLS is the table of calls, each at its smallest shape that still has structure, with every optional output asked
for; a call that takes a slot runs on slot 0 and on slot 1 and returns both answers.

  (a) every ordered pair (A, B) of CALLS, A = B included, on the shared engine and both candidate sets: B's complete output is bit
      for bit the one of a fresh context that ran the writers, gpbo_posterior for the slots B reads a posterior from, and B.  Each
      fresh output is held once to its sibling's truth at that sibling's bar (two runs could be wrong in the same way), and differs
      between the candidate sets and between the slots (a stale answer from the other state would not pass).
  (b) grow, shrink, regrow: each workspace and ctx->red taken from a small layout to the largest the siblings use and back.
  (c) the candidate writers against the new readers: after a writer, mes / kg / ehvi raise the STATE error, the path calls answer as
      a fresh context with the same rows; the trust-region generator after the calls that leave most in ctx->red is the truth's rows.
  (d) stale but refreshable (posterior resident, then gpbo_fit_append: where a batch loop sits between picks): every path call
      leaves the next gpbo_posterior_refresh on its incremental route with the same bits; mes / kg / ehvi refuse and leave it so.
  (e) after a late refusal (the front overflow behind the kernels) and after a host-side refusal of each entry point, the calls
      answer as on a fresh context.

Equality between two device runs is bitwise (the siblings' bitwise_repeatable tests establish that these paths are deterministic);
rows of fronts_out past a front's size are unspecified (include/gpbo.h) and are left out of it.  No tolerance in this file is new.
No pair was refused by the API: all 11 x 11 pairs run for both sets (ascend_paths and acq_argbest have two modes each)."""
import functools
import json
import os
import time
import types

import numpy as np
import pytest

import ehvi_truth as ET
import kg_truth as KT
import mes_truth as MT
import paths_ascent_truth as AT
import paths_truth as P
import qnei_truth as QT
import test_gpu_constrained_paths as CP
import test_gpu_ehvi as EH
import test_gpu_kg as KG
import test_gpu_posterior_refresh as PR
import test_gpu_qnehvi as QH
import test_gpu_qnei as QN
import test_gpu_sizes as SZ
import turbo_truth as TT
from bayesianoptimization_amd import _lib, sobol_tables
from bayesianoptimization_amd._lib import dptr, iptr
from bayesianoptimization_amd.engine import GpEngine
from bayesianoptimization_amd.multiobjective import box_decomposition
from bayesianoptimization_amd.thompson import spectral_draw
from conftest import rel_err
from oracle import gp_oracle as O
from test_gpu_call_order import R, W, replay, replay_fresh      # (W and R make its Steps)

pytestmark = pytest.mark.gpu

CASE = "n130+65-m257-f65-d5-3x16-p64"
Y_MEAN, Y_STD = QH.Y_MEAN, QH.Y_STD
D, GROUP_S = 5, 16
UCB_K = 2.576
KEY = 0x1234567_89ABCDEF
#: GPBO_ERR_STATE of a reader whose slot has no posterior over the current candidates
NO_POSTERIOR = (_lib.GpboError, r"run gpbo_posterior for")

#: worst error / bar per fresh-side truth check and wall seconds per scenario, written as JSON to the file
#: GPBO_CALL_ORDER_SAMPLING_REPORT names (if set) at the end of the module
WORST, SECONDS = {}, {}


def record(what, ratio):
    WORST[what] = max(float(ratio), WORST.get(what, 0.0))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    out = os.environ.get("GPBO_CALL_ORDER_SAMPLING_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump({"worst_error_over_bar": dict(sorted(WORST.items())), "seconds": SECONDS}, f, indent=1)


# ---- the base state -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base():
    return QH.case_of(CASE)


@functools.lru_cache(maxsize=None)
def candidates(tag):
    """"A": the case's own 257; "B": 1024; "L": 4099, the large layout of scenario (b)"""
    if tag == "A":
        return base().Xc
    M = {"B": 1024, "L": 4099}[tag]
    return np.random.RandomState(M).uniform(size=(M, D))


def draws(j, G, S):
    """the first S draws of slot j's first G groups"""
    return [(o, p, w[:S], e[:S]) for o, p, w, e in base().slots[j].groups[:G]]


def rows_of(G, S):
    """their rows in the case's (T, .) references"""
    return [g * GROUP_S + s for g in range(G) for s in range(S)]


@functools.lru_cache(maxsize=None)
def big_draws(j):
    """3 groups of 16 draws over F = 257 features for slot j: the large layout of scenario (b)"""
    s = base().slots[j]
    rs = np.random.RandomState(7000 + j)
    out = []
    for _ in range(3):
        omega, phase = spectral_draw(s.kind, 257, D, rs)
        out.append((omega, phase, rs.standard_normal((16, 257)), rs.standard_normal((16, s.N)) * np.sqrt(QH.NOISE + s.white)))
    return out


@functools.lru_cache(maxsize=None)
def ref_values(tag):
    """((2, T, M) reference of the case's draws at the candidates of `tag`, its bar per objective): QH.Case.references' rule"""
    c = base()
    if tag == "A":
        return c.ref[:, :, :c.M], list(c.bar)
    pts = candidates(tag)
    cho = np.stack([s.route(P.paths_cho, pts) for s in c.slots])
    other = np.stack([s.route(P.paths_winv, pts) for s in c.slots])
    return cho, [max(QH.BAR, QH.MARGIN * QH.err_of(cho[j], other[j], j)) for j in range(2)]


def writers(tag):
    """the writers that make the base state over the candidates of `tag`"""
    c = base()
    return [W(lambda e: c.slots[0].fit(e)), W(lambda e: c.slots[1].fit(e)), W("set_candidates", candidates(tag))]


def posteriors(slots=(0, 1)):
    return [R("posterior", j, Y_MEAN[j], Y_STD[j], check=f"post {j}") for j in slots]


# ---- the calls ------------------------------------------------------------------------------------------------------------------------
def sample_paths(eng, j=0, S=3):
    o, p, w, e = draws(j, 1, S)[0]
    return eng.sample_paths(o, p, w, e, slot=j, y_mean=Y_MEAN[j], y_std=Y_STD[j], return_values=True)


CON_LB, CON_UB = np.array([-1.5]), np.array([0.0])         # slot 1's draws spread about y_mean = -1 with y_std = 2: a part is feasible


def sample_paths_constrained(eng, S=3):
    return eng.sample_paths_constrained([draws(0, 1, S)[0], draws(1, 1, S)[0]], CON_LB, CON_UB, np.array(Y_MEAN), np.array(Y_STD),
                                        return_values=True)


BOX_LO, BOX_HI = np.zeros(D), np.ones(D)
STARTS = np.random.RandomState(31).uniform(size=(3, 2, D))


def ascend_paths(eng, j, given, S=3):
    o, p, w, e = draws(j, 1, S)[0]
    kw = {"starts": STARTS[:S]} if given else {"starts": None, "n_starts": 2}
    return eng.ascend_paths(o, p, w, e, BOX_LO, BOX_HI, slot=j, y_mean=Y_MEAN[j], y_std=Y_STD[j], return_gradient=True, **kw)


Y_STAR = Y_MEAN[0] + Y_STD[0] * np.linspace(0.5, 3.0, 8)


def mes_argbest(eng):
    return eng.mes_argbest(Y_STAR, k_seeds=8, return_values=True)


def kg_points(J=9):
    return np.random.RandomState(41).uniform(size=(64, D))[:J]


def kg_argbest(eng, J=9):
    return eng.kg_argbest(kg_points(J), k_seeds=8, y_mean=Y_MEAN[0], y_std=Y_STD[0], return_values=True, return_point_means=True)


@functools.lru_cache(maxsize=None)
def ehvi_boxes(n=5):
    """a front of n points about the two objectives' means (raw units), its reference point two y_std below them"""
    ym, ys = np.array(Y_MEAN), np.array(Y_STD)
    front = (ym - 0.5 * ys) + 2.0 * ys * ET.random_front(n, 2, n, lo=0.0, hi=1.0)
    return box_decomposition(front, ym - 2.0 * ys)


def ehvi_argbest(eng, n=5):
    n_levels, levels, lo, hi = ehvi_boxes(n)
    return eng.ehvi_argbest(levels, lo, hi, k_seeds=8, return_values=True)


def pending_points():
    c = base()
    return c.base[c.slots[0].N:c.slots[0].N + 3]


def qnei_greedy(eng, j=0, q=3, groups=None, pending=None):
    return eng.qnei_greedy(draws(j, 2, 2) if groups is None else groups, q, pending=pending_points() if pending is None else pending,
                           slot=j, y_mean=Y_MEAN[j], y_std=Y_STD[j], return_values=True, return_keys=True)


def qnehvi_greedy(eng, q=3, both=None):
    c = base()
    out = eng.qnehvi_greedy([draws(0, 2, 2), draws(1, 2, 2)] if both is None else both, q, c.refp, base=c.base, y_mean=Y_MEAN, y_std=Y_STD,
                            return_values=True, return_keys=True, return_fronts=True)
    live = np.arange(out["fronts"].shape[2])[None, None, :] < out["front_size"][:, :, None]
    out["fronts"] = np.where(live[..., None], out["fronts"], 0.0)      # rows past a front's size are unspecified (include/gpbo.h)
    return out


def acq_argbest(eng, k):
    return eng.acq_argbest(O.UCB, UCB_K, k_seeds=k, return_values=True)


def both_slots(fn, *args):
    return lambda eng: tuple(fn(eng, j, *args) for j in (0, 1))


class Call:
    """`run(engine)`: the call's complete output; `entry`: the library function; `needs`: the slots whose resident posterior it reads;
    `per_slot`: it takes a slot, and `run` returns slot 0's and slot 1's answer; `candidates`: it reads the resident candidates
    (ascend_paths with given starts does not: "no candidates are needed", include/gpbo.h)."""

    def __init__(self, entry, run, needs=(), per_slot=False, candidates=True):
        self.entry, self.run, self.needs, self.per_slot, self.candidates = entry, run, tuple(needs), per_slot, candidates


#: the pair matrix of scenario (a) is CALLS x CALLS (module level, no engine call: tests/test_call_order_cover_host.py reads it)
CALLS = {
    "sample_paths": Call("gpbo_sample_paths", both_slots(sample_paths), per_slot=True),
    "sample_paths_constrained": Call("gpbo_sample_paths_constrained", sample_paths_constrained),
    "ascend_paths[resident starts]": Call("gpbo_ascend_paths", both_slots(ascend_paths, False), per_slot=True),
    "ascend_paths[given starts]": Call("gpbo_ascend_paths", both_slots(ascend_paths, True), per_slot=True, candidates=False),
    "mes_argbest": Call("gpbo_mes_argbest", mes_argbest, needs=(0,)),
    "kg_argbest": Call("gpbo_kg_argbest", kg_argbest, needs=(0,)),
    "ehvi_argbest": Call("gpbo_ehvi_argbest", ehvi_argbest, needs=(0, 1)),
    "qnei_greedy": Call("gpbo_qnei_greedy", both_slots(qnei_greedy), per_slot=True),
    "qnehvi_greedy": Call("gpbo_qnhvi_greedy", qnehvi_greedy),
    "acq_argbest[k_seeds=8]": Call("gpbo_acq_argbest", lambda e: acq_argbest(e, 8), needs=(0,)),      # threshold selection
    "acq_argbest[k_seeds=1]": Call("gpbo_acq_argbest", lambda e: acq_argbest(e, 1), needs=(0,)),      # pass selection
}
#: the small layouts of scenario (b): M = 257, S = 1 or T = 4, F = 65
SMALL = {
    "sample_paths": Call("gpbo_sample_paths", lambda e: sample_paths(e, 0, 1)),
    "sample_paths_constrained": Call("gpbo_sample_paths_constrained", lambda e: sample_paths_constrained(e, 1)),
    "ascend_paths[resident starts]": Call("gpbo_ascend_paths", lambda e: ascend_paths(e, 0, False, 1)),
    "ascend_paths[given starts]": Call("gpbo_ascend_paths", lambda e: ascend_paths(e, 0, True, 1)),
    "kg_argbest": Call("gpbo_kg_argbest", kg_argbest, needs=(0,)),
    "ehvi_argbest": Call("gpbo_ehvi_argbest", ehvi_argbest, needs=(0, 1)),
    "qnei_greedy": Call("gpbo_qnei_greedy", lambda e: qnei_greedy(e, 0)),
    "qnehvi_greedy": Call("gpbo_qnhvi_greedy", qnehvi_greedy),
}
#: readers that run between the pairs of scenario (a) and are checked for what they return themselves
BYSTANDERS = ("gpbo_get_alpha", "gpbo_get_candidate_rows", "gpbo_take_negative_variance_flag", "gpbo_lml_batch_scaled")
#: what each scenario calls (library functions), for tests/test_call_order_cover_host.py
SCENARIOS = {
    "a: every ordered pair": tuple(dict.fromkeys(c.entry for c in CALLS.values())) + BYSTANDERS + ("gpbo_posterior",),
    "b: grow, shrink, regrow": tuple(dict.fromkeys(c.entry for c in SMALL.values())) + ("gpbo_acq_argbest", "gpbo_posterior"),
    "c: candidate writers": ("gpbo_generate_candidates_trust_region", "gpbo_set_candidates", "gpbo_generate_candidates",
                             "gpbo_generate_candidates_mt19937", "gpbo_get_candidate_rows", "gpbo_mes_argbest", "gpbo_kg_argbest",
                             "gpbo_ehvi_argbest", "gpbo_sample_paths", "gpbo_qnei_greedy", "gpbo_qnhvi_greedy", "gpbo_acq_argbest"),
    "d: stale but refreshable": ("gpbo_posterior_refresh", "gpbo_fit_append", "gpbo_sample_paths", "gpbo_sample_paths_constrained",
                                 "gpbo_ascend_paths", "gpbo_qnei_greedy", "gpbo_qnhvi_greedy", "gpbo_mes_argbest", "gpbo_kg_argbest",
                                 "gpbo_ehvi_argbest"),
    "e: after a refusal": ("gpbo_qnhvi_greedy", "gpbo_qnei_greedy", "gpbo_sample_paths", "gpbo_acq_argbest",
                           "gpbo_sample_paths_constrained", "gpbo_ascend_paths", "gpbo_mes_argbest", "gpbo_kg_argbest",
                           "gpbo_ehvi_argbest", "gpbo_generate_candidates_trust_region"),
}


def canon(x):
    """An output as something == compares bit for bit (a NaN equals the same NaN, -0.0 is not 0.0)"""
    if x is None:
        return None
    if isinstance(x, dict):
        return tuple((k, canon(x[k])) for k in sorted(x))
    if isinstance(x, (tuple, list)):
        return tuple(canon(v) for v in x)
    a = np.asarray(x)
    return (a.dtype.str, a.shape, a.tobytes())


def first_difference(got, want, path=""):
    """where two outputs differ, for the assertion's message"""
    if isinstance(want, dict):
        for k in want:
            d = first_difference(got[k], want[k], f"{path}[{k!r}]")
            if d:
                return d
        return ""
    if isinstance(want, (tuple, list)):
        for i, (g, w) in enumerate(zip(got, want)):
            d = first_difference(g, w, f"{path}[{i}]")
            if d:
                return d
        return ""
    return "" if canon(got) == canon(want) else f"{path}: {np.asarray(got).ravel()[:4]} != {np.asarray(want).ravel()[:4]}"


def assert_same(got, want, what):
    assert canon(got) == canon(want), f"{what}: not the fresh context's bits at {first_difference(got, want)}"


@functools.lru_cache(maxsize=None)
def fresh(name, tag, table="CALLS"):
    """{"out": the call's output, "post j": (mu, sd)} of a fresh context: the writers, the posteriors the call reads, the call"""
    call = (CALLS if table == "CALLS" else SMALL)[name]
    with GpEngine(0) as eng:
        return replay(eng, writers(tag) + posteriors(call.needs) + [R(call.run, check="out")])


# ---- the fresh side against the siblings' truths ------------------------------------------------------------------------------------
def _check_path_values(what, values, j, tag, rows):
    ref, bar = ref_values(tag)
    e = QH.err_of(values, ref[j][rows], j)
    assert e <= bar[j], f"{what}: error {e:.2e} over its bar {bar[j]:.2e}"
    return e / bar[j]


def _truth_sample_paths(out, tag, post):
    worst = 0.0
    for j, (idx, val, values) in enumerate(out):
        worst = max(worst, _check_path_values(f"sample_paths slot {j} set {tag}", values, j, tag, rows_of(1, 3)))
        assert np.array_equal(idx, np.argmax(values, axis=1)) and np.array_equal(val, values[np.arange(3), idx])
    return worst


def _truth_constrained(out, tag, post):
    shim = types.SimpleNamespace(C=1, y_std=np.array(Y_STD), what=f"sample_paths_constrained set {tag}")
    CP.check_rule(shim, out, CON_LB, CON_UB)
    assert 0.0 < (out[5] == 0.0).mean() < 1.0, "the bounds leave every candidate on one side: this fixture checks nothing"
    return max(_check_path_values(shim.what, out[4][j], j, tag, rows_of(1, 3)) for j in (0, 1))


def _truth_ascend(out, tag, post, given):
    c = base()
    worst = 0.0
    for j, o in enumerate(out):
        s = c.slots[j]
        om, ph, w, e = draws(j, 1, 3)[0]
        args = (s.kind, s.X, s.yn, s.ls, s.eta, om, ph, w, e, o["x"], Y_MEAN[j], Y_STD[j])
        f_ref, g_ref = AT.path_value_grad(*args, amplitude=s.amplitude)
        f2, g2 = AT.path_value_grad(*args, amplitude=s.amplitude, route="winv")
        scale_g = Y_STD[j] * max(1.0, float(np.max(np.abs(g_ref / Y_STD[j]))))
        bar_f = max(QH.BAR, QH.MARGIN * QH.err_of(f2, f_ref, j))
        bar_g = max(QH.BAR, QH.MARGIN * float(np.max(np.abs(g2 - g_ref))) / scale_g)
        ef, eg = QH.err_of(o["f"], f_ref, j), float(np.max(np.abs(o["g"] - g_ref))) / scale_g
        assert ef <= bar_f and eg <= bar_g, f"ascend_paths slot {j} set {tag}: value {ef:.2e} / {bar_f:.2e}, gradient {eg:.2e} / {bar_g:.2e}"
        assert (o["x"] >= BOX_LO).all() and (o["x"] <= BOX_HI).all() and set(np.unique(o["status"])) <= {0, 1, 2, 3}
        assert np.array_equal(o["winner"], np.argmax(o["f"], axis=1)) and np.array_equal(o["f_best"], o["f"].max(axis=1))
        if given:
            assert o["best_idx"] is None and (o["start_idx"] == -1).all()
        else:           # the starts are the draw's two best candidates: sample_paths' answer first
            idx, val, values = fresh("sample_paths", tag)["out"][j]
            assert np.array_equal(o["best_idx"], idx) and np.array_equal(o["best_val"], val) and np.array_equal(o["start_idx"][:, 0], idx)
            assert np.array_equal(o["start_idx"], np.argsort(-values, axis=1, kind="stable")[:, :2])
        worst = max(worst, ef / bar_f, eg / bar_g)
    return worst


def _check_selection(out, k):
    bi, bv, si, sv, ys = out[:5]
    wi, wv, wsi, wsv = MT.argbest(ys, k)
    assert bi == wi and bv == wv and np.array_equal(si, wsi) and np.array_equal(sv, wsv), "the selection is not the values' own"


def _truth_mes(out, tag, post):
    mu, sd = post["post 0"]
    want = -MT.mes_values(mu, sd, Y_STAR)
    worst, ok = MT.within_bar(out[4], want)
    assert ok, f"mes_argbest set {tag}: {worst:.2e} over the bar"
    assert (want < 0).mean() > 0.5, "the truth is zero nearly everywhere: this fixture checks nothing"
    _check_selection(out, 8)
    return worst / MT.BAR


def _truth_kg(out, tag, post):
    s = base().slots[0]
    mu, sd = post["post 0"]
    pts, ys, mu_pts = kg_points(), out[4], out[5]
    want_pts = P.posterior_mean(s.kind, s.X, s.yn, s.ls, s.eta, pts, Y_MEAN[0], Y_STD[0])
    e_pts = float(np.abs(mu_pts - want_pts).max()) / max(1.0, float(np.abs(want_pts).max()))
    assert e_pts <= KT.BAR, f"kg_argbest set {tag}: point means off by {e_pts:.2e}"
    cov = s.amplitude * KT.posterior_cov(s.kind, s.X, s.ls, s.eta, candidates(tag), pts)
    want, scale = KT.kg_values(mu, sd, cov, mu_pts, Y_STD[0], s.white + QH.NOISE, s.white, return_scale=True)
    assert np.mean(want >= 1e-3 * scale) >= 0.10, "the truth is (nearly) zero everywhere: this fixture checks nothing"
    worst = KG.check_values(f"kg_argbest set {tag}", ys, want, scale)
    _check_selection(out, 8)
    return max(worst, e_pts) / KT.BAR


def _truth_ehvi(out, tag, post):
    mu, sd = (np.stack([post[f"post {j}"][i] for j in (0, 1)]) for i in (0, 1))
    n_levels, levels, lo, hi = ehvi_boxes()
    rows = ET.trim(n_levels, levels)
    truth, scale = EH.check_values(f"ehvi_argbest set {tag}", out[4], mu, sd, rows, lo, hi)
    assert np.nanmax(truth) > 0.0
    _check_selection(out, 8)
    return ET.within_bar(-out[4], truth, scale)[0]


def _truth_qnei(out, tag, post):
    c = base()
    worst = 0.0
    n0 = c.slots[0].N
    for j, o in enumerate(out):
        idx, gain, m0, values, keys = o
        what = f"qnei_greedy slot {j} set {tag}"
        worst = max(worst, _check_path_values(what, values, j, tag, rows_of(2, 2)))
        at_base = c.ref[j][rows_of(2, 2)][:, c.M:]                         # the draws at [the 130 observed rows | the 64 pending ones]
        want_m = QT.baseline(at_base[:, :c.slots[j].N], at_base[:, n0:n0 + 3])
        em = QH.err_of(m0, want_m, j)
        assert em <= c.bar[j], f"{what}: baseline error {em:.2e} over its bar {c.bar[j]:.2e}"
        QN.replay(None, o, 3, what)
        worst = max(worst, em / c.bar[j])
    return worst


def _truth_qnehvi(out, tag, post):
    c = base()
    what = f"qnehvi_greedy set {tag}"
    worst = 0.0
    for j in range(2):
        worst = max(worst, _check_path_values(what, out["values"][j], j, tag, rows_of(2, 2)))
        eb = QH.err_of(out["base_values"][j], c.ref[j][rows_of(2, 2)][:, c.M:], j)
        assert eb <= c.bar[j], f"{what}: base values {eb:.2e} over their bar {c.bar[j]:.2e}"
        worst = max(worst, eb / c.bar[j])
    QH.replay(c, out, 3, what)
    assert out["front_size"][0].max() >= 2 and out["front_size"].max() < QH.L
    return worst


def _truth_acq(out, tag, post, k):
    mu, sd = post["post 0"]
    e = rel_err(out[4], -1 * O.base_acq(O.UCB, mu, sd, UCB_K, 0.0))
    assert e <= 1e-8, f"acq_argbest set {tag}: values {e:.2e}"
    _check_selection(out, k)
    return e / 1e-8


TRUTHS = {
    "sample_paths": _truth_sample_paths, "sample_paths_constrained": _truth_constrained,
    "ascend_paths[resident starts]": lambda o, t, p: _truth_ascend(o, t, p, False),
    "ascend_paths[given starts]": lambda o, t, p: _truth_ascend(o, t, p, True),
    "mes_argbest": _truth_mes, "kg_argbest": _truth_kg, "ehvi_argbest": _truth_ehvi, "qnei_greedy": _truth_qnei,
    "qnehvi_greedy": _truth_qnehvi, "acq_argbest[k_seeds=8]": lambda o, t, p: _truth_acq(o, t, p, 8),
    "acq_argbest[k_seeds=1]": lambda o, t, p: _truth_acq(o, t, p, 1),
}


def _core(name, out):
    """the part of an output that must differ between two states: the values over the candidates, and the picks"""
    if CALLS[name].per_slot:
        return tuple(_core_one(name, o) for o in out)
    return _core_one(name, out)


def _core_one(name, o):
    if isinstance(o, dict):
        return canon({k: o[k] for k in ("f", "x", "values", "keys", "index", "gain") if k in o})
    return canon(o)


# ---- (a) every ordered pair ---------------------------------------------------------------------------------------------------------
def _scaled_lml(eng):
    s = base().slots[0]
    return eng.lml_batch_scaled_arrays(s.X, s.yn, s.kind, np.stack([s.ls, 1.1 * s.ls]), [2.5, 1.0], [1e-3, 0.0], QH.NOISE)


@pytest.mark.parametrize("b", list(CALLS))
def test_every_call_before(engine, b):
    """the pairs (A, b) for every A of CALLS, over both candidate sets"""
    t0 = time.perf_counter()
    c, call = base(), CALLS[b]
    for tag in ("A", "B"):
        want = fresh(b, tag)
        record(f"{b}: {tag}", TRUTHS[b](want["out"], tag, want))
        Xc = candidates(tag)
        posts = replay(engine, writers(tag) + posteriors())
        alpha = [engine.get_alpha(s.N, slot=j) for j, s in enumerate(c.slots)]
        lml = _scaled_lml(engine)
        engine.take_negative_variance_flag()
        for a in CALLS:
            CALLS[a].run(engine)
            assert_same(call.run(engine), want["out"], f"{a} then {b} on set {tag}")
        # the readers in between return what they returned before, and nobody clipped a variance
        assert all(np.array_equal(engine.get_alpha(s.N, slot=j), alpha[j]) for j, s in enumerate(c.slots))
        assert np.array_equal(engine.get_candidate_rows(np.arange(Xc.shape[0]), D), Xc)
        assert canon(_scaled_lml(engine)) == canon(lml)
        assert engine.take_negative_variance_flag() is False
        for j in (0, 1):      # ... and the posteriors are still the ones the pass left
            assert_same(engine.posterior(j, Y_MEAN[j], Y_STD[j]), posts[f"post {j}"], f"posterior {j} after the pairs before {b}")
    # a stale answer from the other state could not pass: the sets differ, and the slots
    out_a, out_b = fresh(b, "A")["out"], fresh(b, "B")["out"]
    if call.candidates:
        assert _core(b, out_a) != _core(b, out_b), f"{b}: the same answer over both candidate sets"
    else:
        assert_same(out_a, out_b, f"{b} reads no candidates, sets A and B")
    if call.per_slot:
        for out in (out_a, out_b):
            assert _core_one(b, out[0]) != _core_one(b, out[1]), f"{b}: the same answer for slot 0 and slot 1"
    SECONDS[f"a: {b}"] = round(time.perf_counter() - t0, 2)


# ---- (b) grow, shrink, regrow -------------------------------------------------------------------------------------------------------
def _large(eng):
    """every path-family call at the largest layout the siblings use: M = 4099, S = 16 / T = 48, F = 257, q = 64, 194 base points,
    J = 64 points, a 128-point front"""
    c = base()
    eng.set_candidates(candidates("L"))
    for j in (0, 1):
        eng.posterior(j, Y_MEAN[j], Y_STD[j], fetch=False)
        o, p, w, e = big_draws(j)[0]
        eng.sample_paths(o, p, w, e, slot=j, y_mean=Y_MEAN[j], y_std=Y_STD[j], return_values=True)
        eng.ascend_paths(o, p, w, e, BOX_LO, BOX_HI, n_starts=8, max_iter=3, slot=j, y_mean=Y_MEAN[j], y_std=Y_STD[j])
        eng.ascend_paths(o, p, w, e, BOX_LO, BOX_HI, starts=np.random.RandomState(3).uniform(size=(16, 8, D)), max_iter=3, slot=j,
                         y_mean=Y_MEAN[j], y_std=Y_STD[j])
    eng.sample_paths_constrained([big_draws(0)[0], big_draws(1)[0]], CON_LB, CON_UB, np.array(Y_MEAN), np.array(Y_STD), return_values=True)
    kg_argbest(eng, 64)
    ehvi_argbest(eng, 128)
    qnei_greedy(eng, 0, 64, big_draws(0), c.base[c.slots[0].N:])
    qnehvi_greedy(eng, 64, [big_draws(0), big_draws(1)])


def test_grow_shrink_regrow():
    t0 = time.perf_counter()
    want = {n: fresh(n, "A", "SMALL")["out"] for n in SMALL}
    with GpEngine(0) as eng:
        replay(eng, writers("A") + posteriors())
        first = {n: SMALL[n].run(eng) for n in SMALL}
        _large(eng)
        replay(eng, [W("set_candidates", candidates("A"))] + posteriors())
        again = {n: SMALL[n].run(eng) for n in SMALL}
        for n in SMALL:
            assert_same(first[n], want[n], f"{n}, small, first")
            assert_same(again[n], want[n], f"{n}, small again after the large layout")
        # ctx->red: one-pick records, then records for 65 workgroups x 64 picks (a reallocation), then the small calls again
        qnehvi_greedy(eng)
        big = np.random.RandomState(66).uniform(size=(66000, D))
        eng.set_candidates(big)
        mu, sd = eng.posterior(0, Y_MEAN[0], Y_STD[0])
        out = eng.acq_argbest(O.UCB, UCB_K, k_seeds=64, return_values=True)
        _check_selection(out, 64)
        assert rel_err(out[4], -1 * O.base_acq(O.UCB, mu, sd, UCB_K, 0.0)) <= 1e-8
        eng.set_candidates(candidates("A"))
        assert_same(qnehvi_greedy(eng), want["qnehvi_greedy"], "qnehvi_greedy after the selection records grew")
        assert_same(SMALL["sample_paths"].run(eng), want["sample_paths"], "sample_paths after the selection records grew")
    SECONDS["b"] = round(time.perf_counter() - t0, 2)


# ---- (c) the candidate writers against the new readers ------------------------------------------------------------------------------
def _trust_region(eng, M=257):
    sv, shift = sobol_tables(D, 5)
    args = (M, np.full(D, 0.45), np.full(D, 0.1), np.full(D, 0.9), sv, shift)
    eng.generate_candidates_trust_region(*args, 30, 2 ** 31, KEY)
    return TT.generate(*args, 2 ** 31, KEY)


CANDIDATE_WRITERS = {
    "generate_candidates_trust_region": _trust_region,
    "set_candidates": lambda e: e.set_candidates(candidates("B")[:257]),
    "generate_candidates": lambda e: e.generate_candidates(257, np.zeros(D), np.ones(D), 12345),
    "generate_candidates_like": lambda e: e.generate_candidates_like(257, np.zeros(D), np.ones(D), np.random.RandomState(4)),
}
PATH_READERS = ("sample_paths", "qnei_greedy", "qnehvi_greedy")


@pytest.mark.parametrize("writer", list(CANDIDATE_WRITERS))
def test_candidate_writers_against_the_new_readers(engine, writer):
    t0 = time.perf_counter()
    replay(engine, writers("A") + posteriors())
    CALLS["kg_argbest"].run(engine), CALLS["ehvi_argbest"].run(engine)            # first use behind them: the writer comes after
    truth_rows = CANDIDATE_WRITERS[writer](engine)
    rows = engine.get_candidate_rows(np.arange(257), D)
    if truth_rows is not None:
        assert np.array_equal(rows.view(np.uint64), truth_rows.view(np.uint64)), "the generator's rows are not the truth's"
    assert not np.array_equal(rows, candidates("A"))
    for name in ("mes_argbest", "kg_argbest", "ehvi_argbest"):
        with pytest.raises(NO_POSTERIOR[0], match=NO_POSTERIOR[1]):
            CALLS[name].run(engine)
    got = {n: CALLS[n].run(engine) for n in PATH_READERS}
    with GpEngine(0) as f:
        replay(f, writers("A")[:2] + [W("set_candidates", rows)])
        want = {n: CALLS[n].run(f) for n in PATH_READERS}
    for n in PATH_READERS:
        assert_same(got[n], want[n], f"{n} after {writer}")
        assert _core(n, want[n]) != _core(n, fresh(n, "A")["out"]), f"{n}: the answer over the candidates before {writer}"
    SECONDS[f"c: {writer}"] = round(time.perf_counter() - t0, 2)


def test_trust_region_generator_after_the_calls_that_fill_the_selection_records(engine):
    """ctx->red holds the generator's tables: after the greedy picks' records, after a first-use KG pass, and after the records of a
    64-pick threshold selection, its rows are the truth's bit for bit"""
    t0 = time.perf_counter()
    for name, run in (("qnehvi_greedy", qnehvi_greedy), ("kg_argbest", kg_argbest), ("acq_argbest", lambda e: acq_argbest(e, 64))):
        replay(engine, writers("A") + posteriors())
        run(engine)
        for M in (257, 4099):
            want = _trust_region(engine, M)
            got = np.vstack([engine.get_candidate_rows(np.arange(i, min(i + 4096, M)), D) for i in range(0, M, 4096)])
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"after {name}, M = {M}"
    SECONDS["c: generator after"] = round(time.perf_counter() - t0, 2)


# ---- (d) stale but refreshable --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stale_case(rows):
    """tests/test_gpu_posterior_refresh.py's kind of case at this file's d and M, `rows` rows appended; draws for the grown model"""
    c = PR.Case(130, D, 257, rows, True, PR.F.MATERN25)
    c.mu_o, c.sd_o = c.truth(c.N)
    rs = np.random.RandomState(90 + rows)
    omega, phase = spectral_draw(c.kind, 65, D, rs)
    c.draw = (omega, phase, rs.standard_normal((2, 65)), rs.standard_normal((2, c.N)) * np.sqrt(PR.NOISE))
    return c


def _stale_calls(c):
    """name -> call in the stale state: slot 0 is the grown model (its y_mean / y_std those of the append), slot 1 the base case's"""
    ym, ys = c.norm(c.N)[1:]
    d0, d1 = c.draw, draws(1, 1, 2)[0]
    kw = dict(y_mean=ym, y_std=ys)
    both = dict(y_mean=(ym, Y_MEAN[1]), y_std=(ys, Y_STD[1]))
    return {
        "sample_paths": lambda e: e.sample_paths(*d0, return_values=True, **kw),
        "sample_paths_constrained": lambda e: e.sample_paths_constrained([d0, d1], CON_LB, CON_UB, np.array(both["y_mean"]),
                                                                         np.array(both["y_std"]), return_values=True),
        "ascend_paths[resident starts]": lambda e: e.ascend_paths(*d0, BOX_LO, BOX_HI, n_starts=2, **kw),
        "ascend_paths[given starts]": lambda e: e.ascend_paths(*d0, BOX_LO, BOX_HI, starts=STARTS[:2], **kw),
        "qnei_greedy": lambda e: e.qnei_greedy([d0, d0], 3, pending=pending_points(), return_values=True, return_keys=True, **kw),
        "qnehvi_greedy": lambda e: e.qnehvi_greedy([[d0, d0], [d1, d1]], 3, [ym - ys, Y_MEAN[1] - Y_STD[1]], base=c.X[:c.N],
                                                   return_values=True, return_keys=True, return_fronts=True, **both),
    }


def _stale_refusals(c):
    ym, ys = c.norm(c.N)[1:]
    return {"mes_argbest": mes_argbest, "ehvi_argbest": ehvi_argbest,
            "kg_argbest": lambda e: e.kg_argbest(kg_points(), k_seeds=8, y_mean=ym, y_std=ys, return_values=True)}


@pytest.mark.parametrize("rows", [1, 5])
def test_stale_but_refreshable_survives_the_path_calls(engine, rows):
    t0 = time.perf_counter()
    c = stale_case(rows)
    slot1 = base().slots[1]

    def stale():
        PR.arm(engine, c)
        slot1.fit(engine)
        engine.posterior(1, Y_MEAN[1], Y_STD[1], fetch=False)
        return PR.append(engine, c, c.N0, c.N)

    ym, ys = stale()
    mu, sd, route = engine.posterior_refresh(0, ym, ys, return_route=True)
    assert route == 1
    record(f"d: refresh after {rows} rows, check_posterior 1e-9", SZ.check_posterior(mu, sd, c.mu_o, c.sd_o, ys, c.what + " refresh vs oracle", 1e-9))
    for name, call in {**_stale_calls(c), **_stale_refusals(c)}.items():
        stale()
        if name in _stale_refusals(c):
            with pytest.raises(NO_POSTERIOR[0], match=NO_POSTERIOR[1]):
                call(engine)
        else:
            call(engine)
        mu2, sd2, route2 = engine.posterior_refresh(0, ym, ys, return_route=True)
        assert route2 == route, f"{name} in the stale state: the refresh took route {route2}"
        assert np.array_equal(mu2, mu) and np.array_equal(sd2, sd), f"{name} in the stale state changed the refreshed posterior"
        SZ.check_posterior(mu2, sd2, c.mu_o, c.sd_o, ys, f"{c.what} refresh after {name}", 1e-9)
        # slot 1's posterior was never stale: still the pass's
        assert engine.acq_argbest(O.UCB, UCB_K, 0.0, [-np.inf], [0.0])[0] >= 0
    SECONDS[f"d: {rows} rows"] = round(time.perf_counter() - t0, 2)


# ---- (e) after a refusal --------------------------------------------------------------------------------------------------------------
AFTER = ("qnehvi_greedy", "qnei_greedy", "sample_paths", "acq_argbest[k_seeds=8]")


def _null_draw(eng):
    """gpbo_sample_paths with a NULL omega, at the C boundary"""
    o, p, w, e = (np.ascontiguousarray(a) for a in draws(0, 1, 3)[0])
    bi, bv = np.empty(3, dtype=np.int64), np.empty(3)
    rc = eng._lib.gpbo_sample_paths(eng._h, 0, Y_MEAN[0], Y_STD[0], 3, o.shape[0], None, dptr(p), dptr(w), dptr(e), 0, iptr(bi), dptr(bv), None)
    assert rc == _lib.ERR_INVALID


def _pending_slot(eng):
    """gpbo_sample_paths while a fit is pending on its slot (the engine would wait for it: asked at the C boundary).  Slot 1: a scaled
    fit, as slot 0's, is never left pending (it completes inside its fit() call)"""
    s = base().slots[1]
    o, p, w, e = (np.ascontiguousarray(a) for a in draws(1, 1, 3)[0])
    bi, bv = np.empty(3, dtype=np.int64), np.empty(3)
    with eng.overlapped_fits():
        s.fit(eng)
        rc = eng._lib.gpbo_sample_paths(eng._h, 1, Y_MEAN[1], Y_STD[1], 3, o.shape[0], dptr(o), dptr(p), dptr(w), dptr(e), 0, iptr(bi), dptr(bv), None)
        assert rc == _lib.ERR_STATE


def _overflow(eng):
    """the 129-point anti-diagonal of test_fronts_on_raw_values: refused behind the kernels"""
    diag = lambda n: [[float(k), float(n + 1 - k)] for k in range(1, n + 1)]      # noqa: E731
    with pytest.raises(NotImplementedError, match="draw 1 outgrew 128"):
        QH._debug_fronts(eng, [diag(128) + [[0.5, 0.5]], diag(129)], np.array([0.0, 0.0]))


def _raises(exc, match, fn):
    def run(eng):
        with pytest.raises(exc, match=match):
            fn(eng)
    return run


def _bad_front(eng):
    n_levels, levels, lo, hi = ehvi_boxes()
    eng.ehvi_argbest(levels, hi, lo)


REFUSALS = {
    "qnehvi front overflow (late)": _overflow,
    "sample_paths: NULL draw": _null_draw,
    "sample_paths: slot pending": _pending_slot,
    "sample_paths_constrained: NaN bound": _raises(ValueError, "bounds", lambda e: e.sample_paths_constrained(
        [draws(0, 1, 3)[0], draws(1, 1, 3)[0]], [np.nan], CON_UB, np.array(Y_MEAN), np.array(Y_STD))),
    "ascend_paths: n_starts": _raises(ValueError, "n_starts", lambda e: e.ascend_paths(*draws(0, 1, 3)[0], BOX_LO, BOX_HI, n_starts=9)),
    "mes_argbest: y_star": _raises(ValueError, "finite", lambda e: e.mes_argbest([np.inf])),
    "kg_argbest: points": _raises(ValueError, "finite", lambda e: e.kg_argbest(np.full((2, D), np.nan), y_mean=Y_MEAN[0], y_std=Y_STD[0])),
    "ehvi_argbest: cells": _raises(ValueError, "lo < hi", _bad_front),
    "qnei_greedy: q > M": _raises(ValueError, "q exceeds", lambda e: (e.set_candidates(candidates("A")[:2]), qnei_greedy(e))),
    "qnehvi_greedy: q > M": _raises(ValueError, "q exceeds", lambda e: (e.set_candidates(candidates("A")[:2]), qnehvi_greedy(e))),
    "generate_candidates_trust_region: M": _raises(ValueError, "generate_candidates_trust_region", lambda e: _trust_region(e, 0)),
}


def test_after_a_refusal_the_calls_answer_as_on_a_fresh_context(debug_engine):
    t0 = time.perf_counter()
    eng = debug_engine
    state = writers("A") + posteriors((0,))
    steps = state + [R(CALLS[n].run, check=n, needs=("post 0",)) for n in AFTER]
    want = replay_fresh(steps, debug=True)
    for what, refuse in REFUSALS.items():
        replay(eng, state)
        refuse(eng)
        got = replay(eng, ([] if "q > M" not in what and "pending" not in what else state) + steps[len(state):])
        for n in AFTER:
            assert_same(got[n], want[n], f"{n} after the refusal '{what}'")
    SECONDS["e"] = round(time.perf_counter() - t0, 2)
