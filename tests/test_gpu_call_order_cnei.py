"""GPU (-m gpu): gpbo_cnei_greedy in the order-of-calls contract, in the manner of tests/test_gpu_call_order_sampling.py and over
its base state (two fitted slots — slot 0 the objective, slot 1 the constraint —, the candidate sets A (257) and B (1024)).

  a. gpbo_cnei_greedy before and after each other reader of the path family (CS.CALLS' sample_paths, sample_paths_constrained,
     ascend_paths with resident and with given starts, qnei_greedy, qnehvi_greedy) on ONE context gives the bits a fresh context
     gives — and so does the other call: they share ctx->paths, ctx->Xcs, ctx->ys and the selection's records, the three greedy
     calls lay their workspaces out in ONE buffer (ctx->greedy) and the constrained sampler keeps its own (ctx->cpaths); what one
     call leaves in either must not leak into the next.
  b. after a writer of the candidates (set_candidates) or of a slot (a refit of the constraint's slot on other targets) it answers
     for the new state: the fresh context's bits for that state, which differ from the old state's.

SCENARIOS lists the library functions each scenario runs; tests/test_call_order_cover_ext_host.py holds it against the trailing
section of include/gpbo.h."""
import functools

import numpy as np
import pytest

import test_gpu_call_order_sampling as CS
from bayesianoptimization_amd.engine import GpEngine
from test_gpu_call_order import R, W, replay

pytestmark = pytest.mark.gpu

#: the other readers of the path family, by their names in CS.CALLS
PATH_FAMILY = ("sample_paths", "sample_paths_constrained", "ascend_paths[resident starts]", "ascend_paths[given starts]",
               "qnei_greedy", "qnehvi_greedy")
#: what each scenario calls (library functions), for tests/test_call_order_cover_ext_host.py (module level, no engine call)
SCENARIOS = {
    "a: before and after each path reader": ("gpbo_cnei_greedy",) + tuple(dict.fromkeys(CS.CALLS[n].entry for n in PATH_FAMILY)),
    "b: after a writer": ("gpbo_cnei_greedy", "gpbo_set_candidates", "gpbo_fit"),
}
Y_FLOOR = CS.Y_MEAN[0] - CS.Y_STD[0]


@pytest.fixture(scope="module")
def engine():
    eng = GpEngine(0)
    yield eng
    eng.close()


def cnei_greedy(eng, q=3):
    c = CS.base()
    return eng.cnei_greedy([CS.draws(0, 2, 2), CS.draws(1, 2, 2)], q, CS.CON_LB, CS.CON_UB, Y_FLOOR, base=c.base, y_mean=CS.Y_MEAN,
                           y_std=CS.Y_STD, return_values=True, return_keys=True)


def refit_constraint(eng):
    """the constraint's slot on other targets: every draw of it changes"""
    s = CS.base().slots[1]
    kw = {"amplitude": s.amplitude, "white": s.white} if (s.amplitude, s.white) != (1.0, 0.0) else {}
    eng.fit(s.X, -s.yn, s.kind, s.ls, CS.QH.NOISE, slot=1, **kw)


@functools.lru_cache(maxsize=None)
def fresh(tag, refit=False):
    with GpEngine(0) as eng:
        steps = CS.writers(tag) + ([W(refit_constraint)] if refit else []) + [R(cnei_greedy, check="out")]
        return replay(eng, steps)["out"]


def core(out):
    return CS.canon((out["index"], out["gain"], out["feasible"], out["baseline"]))


@pytest.mark.parametrize("b", PATH_FAMILY)
def test_before_and_after_each_path_reader(engine, b):
    call = CS.CALLS[b]
    for tag in ("A", "B"):
        want, want_b = fresh(tag), CS.fresh(b, tag)["out"]
        replay(engine, CS.writers(tag) + CS.posteriors(call.needs))
        CS.assert_same(cnei_greedy(engine), want, f"cnei_greedy first on set {tag}")
        CS.assert_same(call.run(engine), want_b, f"cnei_greedy then {b} on set {tag}")
        CS.assert_same(cnei_greedy(engine), want, f"{b} then cnei_greedy on set {tag}")
        CS.assert_same(call.run(engine), want_b, f"cnei_greedy then {b} again on set {tag}")
    # a stale answer from the other candidate set could not pass
    assert core(fresh("A")) != core(fresh("B"))
    assert 0.0 < np.mean(fresh("A")["viol"] == 0.0) < 1.0, "the constraint decides nothing over set A: the bounds need another look"


def test_after_a_writer_it_answers_for_the_new_state(engine):
    replay(engine, CS.writers("A"))
    CS.assert_same(cnei_greedy(engine), fresh("A"), "set A")
    engine.set_candidates(CS.candidates("B"))                       # a writer of the candidates
    CS.assert_same(cnei_greedy(engine), fresh("B"), "set B after set A")
    refit_constraint(engine)                                        # a writer of a slot
    CS.assert_same(cnei_greedy(engine), fresh("B", True), "set B after the constraint's refit")
    engine.set_candidates(CS.candidates("A"))
    CS.assert_same(cnei_greedy(engine), fresh("A", True), "set A after the constraint's refit")
    assert core(fresh("B")) != core(fresh("B", True)) and core(fresh("A")) != core(fresh("A", True))
    assert CS.canon(fresh("A")["values"][0]) == CS.canon(fresh("A", True)["values"][0])      # the objective's draws did not change
    assert CS.canon(fresh("A")["viol"]) != CS.canon(fresh("A", True)["viol"])
