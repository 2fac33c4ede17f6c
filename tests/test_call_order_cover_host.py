"""CPU: every entry point has a place in the order-of-calls contract, and every reader is exercised by it.

TABLE classifies every function include/gpbo.h declares outside its GPBO_DEBUG block as a writer of a slot, a writer of the
candidates, a reader, or a call that touches no per-context model or candidate state.  The test fails when a declared function is
missing from the table (or the table names one that is gone), and when a reader appears in no scenario list of
tests/test_gpu_call_order.py and tests/test_gpu_call_order_sampling.py — the next entry point cannot be added without deciding which
it is.  The scenario lists are the two modules' own module-level tables (SCENARIOS), imported; the sampling file's pair matrix is its
CALLS table, whose entries must all be among them.

And the guards of scenario (a) that rest on the reference alone: a call's answer over candidate set A and over set B, and for slot 0
and slot 1, must differ for the bitwise comparison with a fresh context to notice a stale answer from the other state.  Asserted
here on the truths (paths_truth's draws, the oracle's posterior), not on what the device gives."""
import os
import re

import numpy as np

import scaled_kernel_truth as SK
import test_gpu_call_order as CO
import test_gpu_call_order_sampling as CS
from conftest import ROOT

SLOT, CANDIDATES, READER, NEUTRAL = "writer of a slot", "writer of the candidates", "reader", "not per-context state"

TABLE = {
    # lifecycle, errors, instrumentation: no model, posterior or candidate state
    "gpbo_abi_version": NEUTRAL, "gpbo_device_count": NEUTRAL, "gpbo_create": NEUTRAL, "gpbo_destroy": NEUTRAL,
    "gpbo_last_error": NEUTRAL, "gpbo_synchronize": NEUTRAL, "gpbo_device_info": NEUTRAL, "gpbo_last_timings": NEUTRAL,
    "gpbo_set_timing": NEUTRAL, "gpbo_mt19937_jump_blocks": NEUTRAL,
    "gpbo_mfma_f64_peak": NEUTRAL, "gpbo_mfma_f64_probe": NEUTRAL, "gpbo_hbm_copy_peak": NEUTRAL,
    # the fit of a slot
    "gpbo_fit": SLOT, "gpbo_fit_scaled": SLOT, "gpbo_fit_append": SLOT, "gpbo_fit_begin": SLOT, "gpbo_fit_wait": SLOT,
    "gpbo_lml": SLOT, "gpbo_lml_scaled": SLOT,
    # the resident candidates (gpbo_predict* leave THEIR points in the candidate buffer)
    "gpbo_set_candidates": CANDIDATES, "gpbo_generate_candidates": CANDIDATES, "gpbo_generate_candidates_mt19937": CANDIDATES,
    "gpbo_generate_candidate_rows_mt19937": CANDIDATES, "gpbo_generate_candidates_trust_region": CANDIDATES,
    "gpbo_generate_candidate_columns_mt19937": CANDIDATES, "gpbo_set_candidate_columns": CANDIDATES,
    "gpbo_transform_candidates": CANDIDATES, "gpbo_predict": CANDIDATES, "gpbo_predict_cov": CANDIDATES,
    "gpbo_predict_grad": CANDIDATES,
    # readers (the one-launch searches among them: tests/test_gpu_call_order.py's definition)
    "gpbo_polish_seeds": READER, "gpbo_evolve_mixed": READER,
    "gpbo_lml_batch": READER, "gpbo_lml_batch_scaled": READER, "gpbo_get_K": READER, "gpbo_get_L": READER, "gpbo_get_Linv": READER,
    "gpbo_get_alpha": READER, "gpbo_get_candidate_rows": READER, "gpbo_posterior": READER, "gpbo_posterior_refresh": READER,
    "gpbo_sample_paths": READER, "gpbo_sample_paths_constrained": READER, "gpbo_ascend_paths": READER,
    "gpbo_take_negative_variance_flag": READER, "gpbo_acq_argbest": READER, "gpbo_mes_argbest": READER, "gpbo_kg_argbest": READER,
    "gpbo_ehvi_argbest": READER, "gpbo_qnei_greedy": READER, "gpbo_qnhvi_greedy": READER,
    # one process per GPU and device groups: their own handles and tests (tests/test_gpu_sharded.py, tests/test_distributed_gloo.py);
    # a single-GPU scenario cannot drive them
    "gpbo_comm_unique_id": NEUTRAL, "gpbo_comm_init": NEUTRAL, "gpbo_comm_acq_argbest": NEUTRAL, "gpbo_comm_allgather_best": NEUTRAL,
    "gpbo_comm_allreduce_max": NEUTRAL, "gpbo_comm_destroy": NEUTRAL,
    "gpbo_group_create": NEUTRAL, "gpbo_group_destroy": NEUTRAL, "gpbo_group_size": NEUTRAL, "gpbo_group_collective": NEUTRAL,
    "gpbo_group_last_error": NEUTRAL, "gpbo_group_synchronize": NEUTRAL, "gpbo_group_fit": NEUTRAL, "gpbo_group_fit_append": NEUTRAL,
    "gpbo_group_lml_batch": NEUTRAL, "gpbo_group_set_candidates": NEUTRAL, "gpbo_group_shard": NEUTRAL,
    "gpbo_group_generate_candidates_mt19937": NEUTRAL, "gpbo_group_posterior": NEUTRAL, "gpbo_group_acq_argbest": NEUTRAL,
    "gpbo_group_get_candidate_rows": NEUTRAL,
}


def declared():
    """the functions include/gpbo.h declares before its GPBO_DEBUG block"""
    with open(os.path.join(ROOT, "include", "gpbo.h")) as f:
        text = f.read()
    head, sep, _ = text.partition("#ifdef GPBO_DEBUG")
    assert sep, "include/gpbo.h has no GPBO_DEBUG block any more: this test's notion of a debug entry point needs another rule"
    names = re.findall(r"^(?:int|const char\*|void)\s+(gpbo_\w+)\s*\(", head, flags=re.M)
    assert len(names) > 60 and len(set(names)) == len(names)
    return names


def test_every_declared_function_is_classified():
    names = declared()
    assert not [n for n in names if "debug" in n]
    missing = [n for n in names if n not in TABLE]
    gone = [n for n in TABLE if n not in names]
    assert not missing, f"decide what these are in the order-of-calls contract and add them to TABLE: {missing}"
    assert not gone, f"TABLE names functions include/gpbo.h no longer declares: {gone}"
    assert set(TABLE.values()) == {SLOT, CANDIDATES, READER, NEUTRAL}


def test_every_reader_is_in_a_scenario():
    covered = set()
    for module in (CO, CS):
        assert isinstance(module.SCENARIOS, dict) and module.SCENARIOS
        for calls in module.SCENARIOS.values():
            covered.update(calls)
    unknown = sorted(n for n in covered if n not in TABLE)
    assert not unknown, f"the scenario lists name functions that are not declared: {unknown}"
    bare = sorted(n for n, kind in TABLE.items() if kind == READER and n not in covered)
    assert not bare, f"readers that no call-order scenario runs: {bare}"
    # the pair matrix is made of readers, all of them listed
    entries = {c.entry for c in CS.CALLS.values()}
    assert entries <= set(CS.SCENARIOS["a: every ordered pair"]) and all(TABLE[e] == READER for e in entries)
    assert len(CS.CALLS) == 11 and set(CS.SMALL) <= set(CS.CALLS)
    for name in ("sample_paths", "sample_paths_constrained", "ascend_paths", "mes_argbest", "kg_argbest", "ehvi_argbest",
                 "qnei_greedy", "qnehvi_greedy", "acq_argbest"):
        assert any(k.split("[")[0] == name for k in CS.CALLS), name
    assert set(CS.TRUTHS) == set(CS.CALLS)


def test_the_states_differ_on_the_truths_alone():
    """what scenario (a)'s "outputs differ between states" guards rest on: the draws' values, their maxima and maximisers differ
    between the candidate sets and between the slots; so do the oracle's posteriors, which mes / kg / ehvi / acq_argbest read"""
    c = CS.base()
    ref = {tag: CS.ref_values(tag)[0] for tag in ("A", "B")}
    rows = CS.rows_of(2, 2)
    for j in (0, 1):
        best = {tag: ref[tag][j][rows].max(axis=1) for tag in ref}
        arg = {tag: ref[tag][j][rows].argmax(axis=1) for tag in ref}
        span = float(np.ptp(ref["A"][j]))
        assert (np.abs(best["A"] - best["B"]) > 1e-6 * span).all() and (arg["A"] != arg["B"]).any(), f"slot {j}: sets A and B"
    for tag in ref:
        a, b = ref[tag][0][rows], ref[tag][1][rows]
        assert (a.argmax(axis=1) != b.argmax(axis=1)).any() and np.abs(a - b).min(axis=1).max() > 1e-3, f"set {tag}: slots 0 and 1"
    post = {}
    for tag in ref:
        for j, s in enumerate(c.slots):
            gp = SK.ScaledGP(s.kind, s.X, s.yn, s.ls, c=s.amplitude, w=s.white, a=CS.QH.NOISE, y_mean=CS.Y_MEAN[j], y_std=CS.Y_STD[j])
            post[tag, j] = SK.predict(gp, CS.candidates(tag))
    for j in (0, 1):
        (mu_a, sd_a), (mu_b, sd_b) = post["A", j], post["B", j]
        ucb_a, ucb_b = mu_a + CS.UCB_K * sd_a, mu_b + CS.UCB_K * sd_b
        assert abs(ucb_a.max() - ucb_b.max()) > 1e-6 * np.ptp(ucb_a) and ucb_a.argmax() != ucb_b.argmax(), f"slot {j}: sets A and B"
    for tag in ref:
        assert np.abs(post[tag, 0][0] - post[tag, 1][0]).min() > 1e-3, f"set {tag}: the slots' means"
