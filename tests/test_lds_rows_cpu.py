"""CPU check of the row plan of k_admm_lds (mixed-graph-admm_amd/csrc/lds_rows.h, plain C++): rows owned with the long W_d^T
rows first (by tail pairs needed -- the default -- or by in-degree), table positions per wave, and the W_d^T table built under
the plan.  tests/cpu/lds_rows_check.cpp checks the
invariants (permutation, order, every real entry below lim[r] and below npos of every owning wave, a replay of the shortened
gather against the full-width sum, bit for bit); this file feeds it the graphs and pins the per-wave counts of bench.py's own
graphs.  Built with AddressSanitizer + UBSan."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

NLEAD = 5      # LDS_NLEAD of lds_args.h


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("rows") / "lds_rows_check")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "cpu", "lds_rows_check.cpp"), "-o", exe])
    return exe


IN_DEGREE, TAIL_CLASS = 1, 2      # ldsrows::Order


def _run(checker, cl, path, steps=400, order=TAIL_CLASS):
    from export_lds_graph import export
    export(np.asarray(cl), path)
    out = subprocess.run([checker, path, str(NLEAD), str(steps), str(order)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK"), out.stdout
    _run.moved = int(re.search(r"rows moved (\d+) of", out.stdout).group(1))
    npos = [int(v) for v in re.search(r"npos:((?: \d+)+)", out.stdout).group(1).split()]
    width, tp, used, total = map(int, re.search(r"width (\d+) tail_pairs (\d+) positions (\d+) of (\d+)", out.stdout).groups())
    return npos, width, tp, used, total


def _in_degrees(cl):
    cl = np.asarray(cl)
    deg = np.zeros(cl.shape[0], dtype=np.int64)
    for i in range(cl.shape[0]):
        for c in cl[i, 1:]:
            if c >= 0 and c != i:
                deg[c] += 1
    return deg


@pytest.mark.parametrize("workload,order,expect", [("cfg2", IN_DEGREE, [9, 5, 4, 3, 9, 8, 5, 4, 3, 9, 6, 5, 4, 3, 2]),
                                                   ("cfg1", IN_DEGREE, [13, 5, 13, 8, 4, 13, 6, 3]),
                                                   ("cfg2", TAIL_CLASS, [9, 5, 5, 5, 9, 9, 5, 5, 5, 9, 7, 5, 5, 5, 5])])
def test_per_wave_counts_of_the_bench_graphs(checker, tmp_path, workload, order, expect):
    """In-degree order: the counts do not depend on how ties are ordered.  Tail-class order (the default): the same three waves
    per time group gather tail pairs (9 pairs of 30 per workgroup), every other wave the five leading entries."""
    import bench
    n, _, cl, _, _, _ = bench.build_problem(workload)
    npos, width, tp, used, total = _run(checker, cl.numpy(), str(tmp_path / f"{workload}.graph"), order=order)
    assert npos == expect
    deg = _in_degrees(cl.numpy())
    assert tp == (max(0, deg.max() - NLEAD) + 1) // 2 and width == NLEAD + 2 * tp
    assert used == sum(expect) and total == len(expect) * width
    if workload == "cfg2":
        assert np.bincount(deg, minlength=10).tolist() == [1, 6, 40, 87, 79, 45, 24, 8, 13, 4]
        assert (used, total) == ((79, 135) if order == IN_DEGREE else (93, 135))
        assert sum((v - NLEAD + 1) // 2 for v in npos if v > NLEAD) == 9          # tail pairs gathered, of 15 * 2


@pytest.mark.parametrize("order", [IN_DEGREE, TAIL_CLASS])
def test_hub_graphs_of_the_census_cover_the_compile_time_tails(checker, tmp_path, order):
    """tail_pairs 0, 1, 2 and 3: the hub's wave needs the whole table, a wave of short rows only the leading entries."""
    import lds_census as lc
    seen = set()
    for k, r in enumerate(r for r in lc.CENSUS if r["kind"] == "uniform"):
        cl, _ = lc.tables_for(r)
        npos, width, tp, used, total = _run(checker, cl.numpy(), str(tmp_path / f"hub{k}.graph"), steps=100, order=order)
        assert tp == lc.tail_pairs(r["indeg"])
        assert npos[0] == r["indeg"] == max(npos)          # the hub is the first row
        assert used <= total and min(npos) <= NLEAD
        seen.add(tp)
    assert {0, 1, 2, 3} <= seen


@pytest.mark.parametrize("order", [IN_DEGREE, TAIL_CLASS])
@pytest.mark.parametrize("n", [64, 128, 100, 307, 331])
def test_wave_boundaries_and_ghost_waves(checker, tmp_path, n, order):
    """N where no wave straddles two time groups (64, 128), where the last wave is mostly ghosts (331: 993 threads + 31
    ghosts, 100: 300 + 20), and the bench's 307."""
    rng = np.random.default_rng(n)
    cl = np.zeros((n, 5), dtype=np.int64)
    for i in range(n):
        nb = [j for j in (i - 1, i + 1, i - 2, i + 2, i - 3, i + 3, i - 4, i + 4) if 0 <= j < n][:4]
        cl[i] = [i] + nb
    for _ in range(n // 5):
        i, j = rng.integers(n, size=2)
        if i != j and j not in cl[i]:
            cl[i, 1 + rng.integers(4)] = j
    npos, width, tp, used, total = _run(checker, cl, str(tmp_path / f"g{n}.graph"), steps=100, order=order)
    deg = _in_degrees(cl)
    key = deg if order == IN_DEGREE else (np.maximum(deg - NLEAD, 0) + 1) // 2
    deg = deg[np.argsort(-key, kind="stable")]
    G = 3
    expect = []
    for w in range((n * G + 63) // 64):
        rows = [t % n for t in range(64 * w, min(64 * w + 64, n * G))]
        expect.append(int(max(deg[r] for r in rows)))
    assert npos == expect
    if n % 64 == 0 and order == IN_DEGREE:   # every time group starts a wave: the counts repeat per group and only fall inside one
        per = n // 64
        assert npos[:per] == npos[per:2 * per] == npos[2 * per:] and npos[:per] == sorted(npos[:per], reverse=True)


def test_gpu_cases_meet_a_permutation(checker, tmp_path):
    """The graphs of tests/test_gpu_lds_row_order.py: the number of rows the C++ plan moves equals what that test computes
    (`rows_moved`) and asserts on; every case is permuted by the in-degree order, the bench graph also by the default order,
    and the hub graphs of the census (their only long row is node 0) are left in node order by the default."""
    import lds_row_order_cases as rc
    for name in rc.CASES:
        c = rc.case(name)
        cl = c["tables"][0].numpy()
        for order in (IN_DEGREE, TAIL_CLASS):
            _run(checker, cl, str(tmp_path / f"{name}_{order}.graph"), steps=50, order=order)
            assert _run.moved == rc.rows_moved(cl, order), (name, order)
            if order == IN_DEGREE or name.startswith("cfg2"):
                assert _run.moved >= c["N"] // 8, (name, order, _run.moved)
            else:
                assert _run.moved == 0, (name, order)
