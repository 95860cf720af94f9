"""The outer-loop schedule of the LDS-resident path (mixed-graph-admm_amd/csrc/lds_schedule.h, plain C++) on the CPU: which
buffer holds iterate k, which metric set and events a chunk uses, and the ring behind the host's late look at a device word.

tests/cpu/lds_schedule_check.cpp (built with AddressSanitizer + UBSan, run as a program of its own) replays the order in
which Engine::solve_lds issues launches, metric kernels, event records and waits, for every max_it in 1 .. 70 and every
chunk request in 1 .. 16 (CHUNKS) and every max_it for SYNC and DEVSTOP, and checks with stream order and the events as the
only happens-before relation:
  a. no launch writes an iterate buffer or a metric set before an earlier read of it;
  b. the event slot a wait names was last recorded by the chunk the wait is meant for (ring reuse of ev_main / ev_side);
  c. the layout: the buffers of a chunk are distinct, only the last iterate is x_out, no slot >= slots(), and J <= 4 needs
     no more than the 15 workspace vectors;
  d. the lagged ring reads at step c what was written at step c - LAG and rewrites no word before it is read;
  e. the same checker reports a hazard on round 3's "two sets, three boundary buffers" with today's wait three chunks back.
It exits with status 1 at the first check that does not hold.

Identity with the parent: tests/golden/lds_schedule_parent.json holds what the commit before the schedule moved out of
engine.h computed -- the text of its expressions for ps_mode, sched, J, xbuf / ring and the event indices, compiled as a
throw-away host program (not kept) -- and the header reproduces it exactly: the schedule only moved."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, PKG, ROOT


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("sched") / "lds_schedule_check")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "cpu", "lds_schedule_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(out.stdout)


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(GOLDEN, "lds_schedule_parent.json")) as f:
        return json.load(f)


def test_no_hazard_in_any_schedule_and_the_checker_can_fail(replay):
    """Checks a - d passed for the whole grid (the program's exit status); e: the wrong variant fails first where a third
    launch exists, at its write of the metric set chunk 0's metrics still read."""
    assert len(replay["rows"]) == 16 + 2
    wrong = replay["wrong_variant"]
    assert wrong["first"] == [3, 1] and wrong["why"].startswith("write before a pending read")
    # every (J, max_it) with more than two chunks: sum over J = 1 .. 16 of max(0, 70 - 2 J)
    assert wrong["hazards"] == sum(max(0, 70 - 2 * j) for j in range(1, 17))


def test_the_header_includes_no_hip_and_reads_no_environment():
    with open(os.path.join(PKG, "csrc", "lds_schedule.h")) as f:
        text = f.read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ['"lds_consts.h"'] and "getenv" not in text


def test_pick_and_lagged_ring_equal_the_parent_commit(replay, parent):
    assert replay["pick"] == parent["pick"] and len(parent["pick"]) == 16
    assert replay["lag"] == parent["lag"] and len(parent["lag"]) == 12


def test_the_recorded_rows_are_these(parent):
    assert sorted(parent["rows"]) == sorted(["SYNC/1", "DEVSTOP/1"] + [f"CHUNKS/{j}" for j in range(1, 17)])


@pytest.mark.parametrize("row", ["SYNC/1", "DEVSTOP/1"] + [f"CHUNKS/{j}" for j in range(1, 17)])
def test_slots_and_events_equal_the_parent_commit(replay, parent, row):
    got, want = replay["rows"][row], parent["rows"][row]
    assert len(want["J"]) == len(want["slots"]) == 70
    for k in ("J", "slots", "iterates", "chunks"):
        assert got[k] == want[k], (row, k)
