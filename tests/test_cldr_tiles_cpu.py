"""CPU check of the fused cLdr kernel's tile tables (mixed-graph-admm_amd/csrc/cldr_tiles.h, plain C++): the checker
tests/cpu/cldr_tiles_check.cpp replays the kernel's dataflow on the host from the tables and compares it with
Ldr^T(Ldr x) taken directly from the CSR matrices (operator definitions of reference ADMM.py:150-228)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("cldr") / "cldr_tiles_check")
    # AddressSanitizer + UBSan build (sanitizers on the CPU-buildable host code): an out-of-range
    # table index in the builder or in the replay aborts the run
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "cpu", "cldr_tiles_check.cpp"), "-o", exe])
    return exe


# n, T, Rcap, C1cap, C2cap, GD, GT, cluster
@pytest.mark.parametrize("args", [
    (3000, 6, 64, 88, 120, 8, 12, 64),     # float32 production geometry
    (3000, 4, 32, 56, 80, 8, 12, 64),      # float64 geometry (clusters are halved to fit)
    (1000, 3, 64, 88, 120, 8, 12, 37),     # tiles not aligned to the caps
    (500, 2, 8, 24, 48, 8, 12, 8),         # tiny tiles, T = 2 (first step is also the one before the last)
    (777, 5, 64, 40, 60, 8, 12, 64),       # tight halo caps force repeated halving
    (64, 7, 64, 88, 120, 8, 12, 64),       # one tile holds the whole graph
])
def test_tile_tables_reproduce_cldr(checker, args):
    out = subprocess.run([checker] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK"), out.stdout


# ------------------------------------------------------------------------------------------------------------------
# The engine's own geometries: the caps come from CLDR_GEOMS in cldr_tiles.h (`g<number>`), the table engine.h builds
# its ClG1 ... ClG4 from, so this file cannot drift away from the kernel's tile sizes again.
import stream_census as sc

GEOM_CAPS = {g: (nw * ma, nw * mq, nw * mp) for g, (_, nw, ma, mq, mp) in sc.CLDR_GEOMS.items()}      # parsed from the header


def _run(checker, args):
    out = subprocess.run([checker] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    head = out.stdout.splitlines()[0]
    m = re.match(r"rows max_d (\d+) rows_of_max_d (\d+) max_t (\d+) caps (\d+) (\d+) (\d+)$", head)
    assert m, out.stdout
    return [int(v) for v in m.groups()], out.stdout


def test_geometry_table_is_the_engines():
    assert GEOM_CAPS == {1: (16, 32, 40), 2: (64, 88, 120), 3: (32, 64, 80), 4: (32, 48, 64)}      # the caps in use today
    eng = open(os.path.join(PKG, "csrc", "engine.h")).read()
    for i in (1, 2, 3, 4):
        assert re.search(r"typedef ClGOf<%d, [^>]+> ClG%d;" % (i, i), eng)
    assert not re.search(r"typedef ClG<\d", eng)              # no second copy of the numbers


# geometry, GD, GT, (n, T, cluster, k, hubs, hub_indeg, stride, row_limit), longest W_d row, range of the longest W_d^T row
GEOM_CASES = [
    # GD = 6 / 8 with W_d rows of 5, 6, 7 and 8 entries, every geometry
    (1, 6, 12, (1000, 5, 64, 4), 5, (6, 12)), (1, 6, 12, (700, 4, 64, 5), 6, (6, 12)),
    (1, 8, 12, (1000, 5, 64, 6), 7, (6, 12)), (1, 8, 12, (1000, 5, 64, 7), 8, (6, 12)),
    (2, 6, 12, (1000, 5, 64, 4), 5, (6, 12)), (2, 8, 12, (1000, 5, 64, 6), 7, (6, 12)), (2, 8, 12, (1000, 5, 64, 7), 8, (6, 12)),
    (3, 6, 12, (1000, 5, 64, 4), 5, (6, 12)), (3, 8, 12, (1000, 5, 64, 6), 7, (6, 12)), (3, 8, 12, (1000, 5, 64, 7), 8, (6, 12)),
    (4, 6, 12, (1000, 5, 64, 4), 5, (6, 12)), (4, 8, 12, (1000, 5, 64, 6), 7, (6, 12)), (4, 8, 12, (1000, 5, 64, 7), 8, (6, 12)),
    # GT = 16: W_d^T rows of 13 ... 16 entries (star hubs), GT = 24: 17 ... 24
    (1, 8, 16, (1000, 5, 64, 6, 3, 8, 0), 7, (13, 16)), (1, 8, 16, (1000, 5, 64, 6, 3, 10, 0), 7, (16, 16)),
    (3, 8, 16, (600, 4, 64, 7, 2, 8, 0), 8, (13, 16)), (3, 8, 16, (600, 4, 64, 7, 2, 11, 0), 8, (13, 16)),
    (4, 8, 16, (1000, 5, 64, 6, 3, 8, 0), 7, (13, 16)), (2, 8, 16, (1000, 5, 64, 6, 3, 10, 0), 7, (16, 16)),
    (1, 8, 24, (1000, 5, 64, 6, 3, 12, 0), 7, (17, 24)), (1, 8, 24, (1000, 5, 64, 6, 3, 19, 0), 7, (24, 24)),
    (1, 6, 24, (600, 4, 64, 5, 2, 15, 0), 6, (17, 24)), (2, 8, 24, (600, 4, 64, 7, 2, 19, 0), 8, (17, 24)),
    (3, 8, 24, (1000, 5, 64, 6, 3, 16, 0), 7, (17, 24)), (4, 8, 24, (1000, 5, 64, 6, 3, 18, 0), 7, (17, 24)),
    # a non-zero row_limit (MGADMM_CLDR_ROWS)
    (1, 8, 12, (1000, 3, 50, 7, 0, 0, 1, 5), 8, (6, 12)), (3, 8, 12, (1000, 3, 64, 6, 0, 0, 1, 20), 7, (6, 12)),
    (2, 8, 12, (1000, 5, 64, 6, 0, 0, 1, 10), 7, (6, 12)),
]


@pytest.mark.parametrize("geom,gd,gt,graph,max_d,t_range", GEOM_CASES)
def test_engine_geometries_reproduce_cldr(checker, geom, gd, gt, graph, max_d, t_range):
    n, T, cluster = graph[:3]
    (got_d, n_max_d, got_t, *caps), text = _run(checker, [n, T, f"g{geom}", gd, gt, cluster] + list(graph[3:]))
    assert tuple(caps) == GEOM_CAPS[geom]
    assert got_d == max_d and n_max_d > n // 2, text                 # most rows have the stated length
    assert t_range[0] <= got_t <= t_range[1], text
    # the slot counts are the ones the engine would pick for these row lengths (cldr_prepare)
    assert gd == (8 if got_d > 6 else 6) and gt == (12 if got_t <= 12 else 16 if got_t <= 16 else 24)
    assert text.strip().endswith("OK"), text
    if len(graph) > 7:
        assert int(re.search(r"maxR (\d+)", text).group(1)) == graph[7], text      # the row limit is reached and kept


def test_cases_cover_every_class():
    assert {(g, d, t) for g, d, t, *_ in GEOM_CASES} >= {(g, 8, t) for g in (1, 2, 3, 4) for t in (12, 16, 24)}
    assert {(g, d) for g, d, *_ in GEOM_CASES} == {(g, d) for g in (1, 2, 3, 4) for d in (6, 8)}
    assert {c[4] for c in GEOM_CASES} == {5, 6, 7, 8}


@pytest.mark.parametrize("args,why", [
    ((1000, 5, "g1", 8, 12, 64, 8), "d9"),                    # a W_d row of 9 entries: more than the 8 slots
    ((1000, 5, "g1", 8, 24, 64, 6, 3, 20, 0), "t25"),         # a W_d^T row of 25 entries: more than the 24 slots
    ((1000, 5, "g1", 8, 24, 64, 7, 1, 20, 5), "caps"),        # one hub row alone: its 2-hop set exceeds the C2 cap
])
def test_graphs_the_fused_kernel_cannot_take(checker, args, why):
    (got_d, _, got_t, *caps), text = _run(checker, args)
    assert text.strip().endswith("INELIGIBLE"), text
    if why == "d9":
        assert got_d == 9 and got_t <= 24
    elif why == "t25":
        assert got_t == 25 and got_d <= 8
    else:
        assert got_d <= 8 and got_t <= 24 and tuple(caps) == GEOM_CAPS[1]      # the rows fit their slots: it is the caps
        # ... and the same graph fits the larger caps of geometry 2
        _, text2 = _run(checker, (args[0], args[1], "g2") + tuple(args[3:]))
        assert text2.strip().endswith("OK"), text2
