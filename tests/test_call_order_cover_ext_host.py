"""CPU: the order-of-calls contract for the entry points include/gpbo.h declares BEHIND its GPBO_DEBUG block — the sibling of
tests/test_call_order_cover_host.py, whose table closes at that block.

TABLE classifies every function of the trailing section as a writer of a slot, a writer of the candidates, a reader, or a call that
touches no per-context model or candidate state.  The test fails when a function declared there is missing from the table (or the
table names one that is gone), and when a reader there appears in no scenario list of tests/test_gpu_call_order_cnei.py — the next
entry point of that section cannot be added without deciding which it is."""
import os
import re

import test_call_order_cover_host as COVER
import test_gpu_call_order_cnei as CC
from conftest import ROOT

SLOT, CANDIDATES, READER, NEUTRAL = COVER.SLOT, COVER.CANDIDATES, COVER.READER, COVER.NEUTRAL

TABLE = {
    "gpbo_cnei_greedy": READER,
}


def declared_behind_the_debug_block():
    with open(os.path.join(ROOT, "include", "gpbo.h")) as f:
        text = f.read()
    _, sep, tail = text.partition("#endif /* GPBO_DEBUG */")
    assert sep, "include/gpbo.h no longer ends its debug block with `#endif /* GPBO_DEBUG */`: this test needs another rule"
    tail = re.sub(r"/\*.*?\*/", "", tail, flags=re.S)
    names = re.findall(r"^(?:int|const char\*|void)\s+(gpbo_\w+)\s*\(", tail, flags=re.M)
    assert len(set(names)) == len(names)
    return names


def test_every_function_of_the_trailing_section_is_classified():
    names = declared_behind_the_debug_block()
    assert names, "the trailing section is empty"
    assert not [n for n in names if "debug" in n]
    missing = [n for n in names if n not in TABLE]
    gone = [n for n in TABLE if n not in names]
    assert not missing, f"decide what these are in the order-of-calls contract and add them to TABLE: {missing}"
    assert not gone, f"TABLE names functions the trailing section no longer declares: {gone}"
    assert set(TABLE.values()) <= {SLOT, CANDIDATES, READER, NEUTRAL}
    # the two tables do not overlap, and the section really sits behind the first table's reach
    assert not set(TABLE) & set(COVER.TABLE) and not set(names) & set(COVER.declared())


def test_every_reader_there_is_in_a_scenario():
    assert isinstance(CC.SCENARIOS, dict) and CC.SCENARIOS
    covered = set()
    for calls in CC.SCENARIOS.values():
        covered.update(calls)
    both = {**COVER.TABLE, **TABLE}
    unknown = sorted(n for n in covered if n not in both)
    assert not unknown, f"the scenario lists name functions that are not declared: {unknown}"
    bare = sorted(n for n, kind in TABLE.items() if kind == READER and n not in covered)
    assert not bare, f"readers of the trailing section that no call-order scenario runs: {bare}"
    # scenario (a) runs it against the other readers of the path family, scenario (b) behind a writer of each kind
    a, b = CC.SCENARIOS["a: before and after each path reader"], CC.SCENARIOS["b: after a writer"]
    for name in ("gpbo_sample_paths", "gpbo_sample_paths_constrained", "gpbo_ascend_paths", "gpbo_qnei_greedy", "gpbo_qnhvi_greedy"):
        assert name in a and both[name] == READER
    assert any(both[n] == SLOT for n in b) and any(both[n] == CANDIDATES for n in b)
