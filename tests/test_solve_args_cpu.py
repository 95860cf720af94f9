"""The Python front end answers the arguments of a solve as the commit before mgadmm/solve_args.py did: every row and every
trace of tests/golden/solve_args_parent.json, recorded from that commit by tests/golden/gen_solve_args.py (which describes
them), is formed again with this tree and compared whole -- exception type and full message, normalised result, the sequence
of ABI calls with their arguments.  None is skipped.  No GPU: the library is replaced by a recording stub."""
import json
import sys

import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)

import gen_solve_args as gen                  # noqa: E402


@pytest.fixture(scope="module")
def parent():
    return gen.load()


@pytest.fixture(scope="module")
def here():
    mp = pytest.MonkeyPatch()
    try:
        return gen.collect(mp)
    finally:
        mp.undo()


@pytest.mark.parametrize("part", ["rows", "traces"])
def test_every_answer_of_the_parent_is_reproduced(parent, here, part):
    assert list(here[part]) == list(parent[part])                  # the same cases, none left out
    differ = [k for k in parent[part] if here[part][k] != parent[part][k]]
    for k in differ[:3]:
        print(k, "\n  parent:", json.dumps(parent[part][k])[:2000], "\n  here:  ", json.dumps(here[part][k])[:2000])
    assert not differ, f"{len(differ)} of {len(parent[part])} {part} differ: {differ[:20]}"


def test_the_fixture_holds_what_the_issue_of_the_refactor_asked_for(parent):
    rows, traces = parent["rows"], parent["traces"]
    assert parent["raise_sites"] == {"total": 62, "hit": 62}       # of the parent: every raise statement outside _device
    n_bad = len(gen.BAD_SP) + len(gen.BAD_SCH) + len(gen.BAD_AR) + len(gen.BAD_GP)
    assert n_bad >= 11 + 17 + 15 + 8 and all(f"{arg} {i} solve" in rows for arg, lst in (
        ("sample_params", gen.BAD_SP), ("param_schedule", gen.BAD_SCH), ("adaptive_rho", gen.BAD_AR), ("graph_params", gen.BAD_GP))
        for i in range(len(lst)))
    assert all("message" in r or "returns" in r for r in rows.values())
    # two refusals due at once, for every adjacent pair of the order of refusals: the earlier one answers
    first = lambda tag: rows[f"pair {tag} solve"]["message"]
    assert first("sample_params+param_schedule").startswith("sample_params['rho'][1]")
    assert first("param_schedule+graph").startswith("param_schedule['rho'] must have shape")
    assert first("graph+adaptive_rho") == "graph_of_sample needs graph_sets"
    assert first("adaptive_rho+exclude").startswith("adaptive_rho: every = 0")
    assert first("exclude+y").startswith("adaptive_rho and param_schedule exclude each other")
    # the 12 admissible combinations, each with every outcome
    assert len(gen.COMBOS) == 12
    for combo in gen.COMBOS:
        tag = "+".join(combo) or "plain"
        for what in ["ok", "solve refused", "non-finite", "warm_start misses a key"] + [f"{nm} refused" for nm in combo]:
            assert f"{tag}: {what}" in traces, (tag, what)
        names = [c[0] for c in traces[f"{tag}: ok"]["calls"]]
        sets = [n for n in names if n in gen.SETTER.values()]
        want = [gen.SETTER[nm] for nm in ("sample_params", "graph_params", "param_schedule", "adaptive_rho") if nm in combo]
        assert sets == want + want[::-1], (tag, sets)              # set in this order, cleared in the reverse one
    assert "two_loops" in traces and all(f"combined_loop: {nm}" in traces for nm in gen.ARGS)


def test_every_raise_statement_of_the_front_end_is_reached(here):
    sites = here["raise_sites"]
    assert sites["missed"] == [] and sites["hit"] == sites["total"] > 0, sites
