"""The planner of the LDS-resident path (mixed-graph-admm_amd/csrc/lds_plan.h, plain C++) on the CPU: which k_admm_lds
instance a graph gets, its geometry, and the image of tables the kernel reads.

tests/cpu/lds_plan_check.cpp runs ldsplan::make on a graph file and prints the plan, the instance and a hash of the image
(built with AddressSanitizer + UBSan).  The graphs are built the way the product builds them up to the point where it hands
them to the library (ADMM_algorithm's tables -> graph.tables_to_csr; the exact transpose of W_d in the order of
csrc/graph.hip, mg_transpose_csr: entries of a row sorted by source row), so no device is needed for any graph kind.

  * census: every row of lds_census.CENSUS, with the row's switches, gets the row's instance, the geometry of
    lds_census.geometry and the tail of lds_census.tail_pairs -- what tests/test_gpu_lds_census.py asserts on the GPU;
  * the fold rule (tests/test_cg_fold_cpu.py): a graph whose second operator is not the exact transpose of W_d never
    gets a uniform-row instance (three barriers per CG iteration, p . A p from q . q);
  * graphs without a plan: no width with N * G <= 1024 threads, or tables that leave no room in 160 KiB of LDS;
  * byte identity: tests/golden/lds_plan_parent.json holds the plan fields and the image hash that Engine::plan_lds of
    the commit before the planner moved out of engine.h gave for the cases of CASES (its text compiled as a host
    program, same compiler and flags).  The planner only moved: every field and every image byte is the same.
    Under the sanitizers the bank search of a wide W_d^T table takes up to 40 s at the default 4000 steps (4 s for cfg2):
    the census rows with a tail of three pairs or more are recorded and compared at SHORT_SEARCH steps, every other case
    at the default, and the cases run side by side.
"""
import json
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import lds_census as lc      # noqa: E402

PLAN_FIELDS = ("ok", "G", "TPG", "TS", "nthreads", "block", "NR", "csr_ints", "maxt", "sb", "uniform45", "slots", "tail_pairs",
               "lds_img0", "lds_img_ints", "off_rp_u", "off_rp_d", "off_en_u", "off_en_d", "off_lead_t", "off_tail_t", "off_diag",
               "row_order", "off_node", "off_rown", "npos_word", "lds_bytes", "image_ints", "image_hash")
PLANNED, NO_PLAN = 0, 1      # ldsplan::Status
SHORT_SEARCH = 400


# ------------------------------------------------------------------------------------------------ graphs
def planner_input(blk):
    """What ADMM_algorithm._graph and mgadmm_graph_create make of a product's tables, without a device:
    dict(T, N, band, tbg, u, d, dT) with CSR triples (rowptr, col, val float32)."""
    from mgadmm.graph import tables_to_csr
    N = blk.n_nodes
    u = tables_to_csr(blk.connect_list, blk._time_invariant(blk.u_ew, "u_ew"), 1)
    if blk.use_line_graph:
        empty = (np.zeros(N + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
        return dict(T=blk.T, N=N, band=1, tbg=0, u=u, d=empty, dT=empty)
    d = tables_to_csr(blk.connect_list, blk._time_invariant(blk.d_ew, "d_ew"), 0)
    if not blk.use_kNN:                                  # transpose_by_gather (quirk Q4): the second operator is W_d itself
        return dict(T=blk.T, N=N, band=0, tbg=1, u=u, d=d, dT=d)
    rowptr, col, val = d
    order = np.argsort(col, kind="stable")               # mg_transpose_csr: a transposed row holds its entries by source row
    src = np.repeat(np.arange(N, dtype=np.int32), np.diff(rowptr))
    rp_t = np.zeros(N + 1, np.int32)
    np.cumsum(np.bincount(col, minlength=N), out=rp_t[1:])
    return dict(T=blk.T, N=N, band=0, tbg=0, u=u, d=d, dT=(rp_t, src[order], val[order]))


def write_graph(g, path):
    with open(path, "w") as f:
        f.write(f"{g['T']} {g['N']} {g['band']} {g['tbg']}\n")
        for rowptr, col, val in (g["u"], g["d"], g["dT"]):
            bits = np.ascontiguousarray(val, dtype=np.float32).view(np.uint32)
            f.write(f"{len(col)}\n" + " ".join(map(str, rowptr)) + "\n" + " ".join(map(str, col)) + "\n"
                    + " ".join(f"{b:08x}" for b in bits) + "\n")


def _census_product(r):
    import test_gpu_lds_census as tc
    return tc._product(r, tc._info(r["N"], r["T"]))


def _bench_product(workload):
    import bench
    import mgadmm
    n, _, cl, dl, info, _ = bench.build_problem(workload)
    return mgadmm.ADMM_algorithm({"n_nodes": n}, info, use_kNN=True, k=4, u_sigma=50, d_sigma=50, tables=(cl, dl))      # bench.make_solver


def _g4_product(mode):
    """The golden k = 4 table without pads (N = 30): 'knn', 'skip3' (band mode), or 'physical' on the kNN table."""
    from helpers import make_product
    import lds_cg_fold_cases as fc
    return make_product(fc.g4_meta(physical_on_knn_tables=mode == "physical"), mode)


def _uniform_product(N, T):
    import mgadmm
    info = dict(rho=1.0, rho_u=1.0, rho_d=1.0, mu_u=1, mu_d1=1, mu_d2=1)
    return mgadmm.ADMM_algorithm({"n_nodes": N}, info, use_kNN=True, k=4, tables=lc.uniform_tables(N, 6), T=T, t_in=T // 2)


def _sw(**kw):
    return {"MGADMM_LDS_" + k: str(v) for k, v in kw.items()}


def _census_name(r):
    return "census" + lc.row_id(r)


def _census_switches(r):
    wide = r["kind"] == "uniform" and lc.tail_pairs(r["indeg"]) >= 3
    return dict(r["env"], **(_sw(BANK_SEARCH=SHORT_SEARCH) if wide else {}))


# name -> (graph key, product builder, switches): the cases recorded in tests/golden/lds_plan_parent.json
CASES = {_census_name(r): (_census_name(r), (lambda r=r: _census_product(r)), _census_switches(r)) for r in lc.CENSUS}
CASES.update({
    "cfg2": ("cfg2", lambda: _bench_product("cfg2"), {}),
    "cfg1": ("cfg1", lambda: _bench_product("cfg1"), {}),
    "g4": ("g4", lambda: _g4_product("knn"), {}),
    "g4_transpose_by_gather": ("g4_physical", lambda: _g4_product("physical"), {}),
    "g4_skip3": ("g4_skip3", lambda: _g4_product("skip3"), {}),
})
CASES.update({"cfg2_" + "_".join(f"{k}{v}" for k, v in sw.items()): ("cfg2", CASES["cfg2"][1], _sw(**sw)) for sw in (
    dict(ROW_ORDER=0), dict(ROW_ORDER=1), dict(TABLE_ORDER=1), dict(BANK_SEARCH=0), dict(TPG=12), dict(RAGGED=1), dict(SB=1),
    dict(NOSLOTS=1))})
assert len(CASES) == 45 + 5 + 8


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """run(graph key, builder, switches) -> the JSON object lds_plan_check prints; graph files are written once per key."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("plan")
    exe = str(tmp / "lds_plan_check")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "cpu", "lds_plan_check.cpp"), "-o", exe])
    files, seen = {}, {}

    def run(key, build, switches):
        if key not in files:
            files[key] = str(tmp / (key.translate({ord(c): "_" for c in "<>,-"}) + ".graph"))
            write_graph(planner_input(build()), files[key])
        args = tuple(f"{k}={v}" for k, v in sorted(switches.items()))
        if (key, args) not in seen:
            env = {k: v for k, v in os.environ.items() if not k.startswith("MGADMM_LDS_")}
            out = subprocess.run([exe, files[key], *args], capture_output=True, text=True, env=env)
            assert out.returncode == 0, (key, args, out.stdout + out.stderr)
            seen[key, args] = json.loads(out.stdout)
        return seen[key, args]
    return run


# ------------------------------------------------------------------------------------------------ census
@pytest.mark.parametrize("r", lc.CENSUS, ids=lc.row_id)
def test_census_row_gets_its_instance_and_geometry(planner, r):
    """Instance, geometry and tail do not depend on the bank search: run without it."""
    p = planner(_census_name(r), lambda: _census_product(r), dict(r["env"], MGADMM_LDS_BANK_SEARCH="0"))
    assert p["status"] == PLANNED and p["ok"] == 1
    assert p["instance_name"] == r["expect"]
    from mgadmm import _lib
    assert _lib.decode_lds_instance(p["instance"]) == r["expect"]
    nth, rows, ts, ghosts = lc.geometry(r)
    assert (p["nthreads"], p["NR"], p["TS"]) == (nth, rows, ts), f"{ghosts} ghosts"
    assert p["block"] - p["nthreads"] == ghosts
    if r["kind"] == "uniform":
        assert p["tail_pairs"] == lc.tail_pairs(r["indeg"])
    assert p["cg_barriers"] == (3 if p["uniform45"] else 4 + p["sb"])
    assert p["uniform45"] == (1 if ", 4, 5, " in r["expect"] else 0) and p["sb"] == (1 if "MGADMM_LDS_SB" in r["env"] else 0)


# ------------------------------------------------------------------------------------------------ fold rule
def test_no_uniform_instance_without_the_exact_transpose(planner):
    """The g4 kNN table (k = 4, no pads) qualifies for the uniform-row instances by its shape.  With transpose_by_gather
    (use_kNN=False) p . A p != sum dc p^2 + c2 |Ldr p|^2 (test_cg_fold_cpu.py), so the plan must be a generic instance."""
    exact = planner("g4", lambda: _g4_product("knn"), {})
    assert exact["uniform45"] == 1 and exact["cg_barriers"] == 3 and exact["TPG"] == 8
    assert exact["instance_name"] == lc.uni(8, 1024, True, exact["tail_pairs"] if exact["tail_pairs"] <= 3 else -1)
    gather = planner("g4_physical", lambda: _g4_product("physical"), {})
    assert gather["uniform45"] == 0 and gather["cg_barriers"] == 4 and gather["row_order"] == 0
    assert gather["instance_name"] == lc.inst(gather["TPG"], False, 1024, False)
    for tpg in (8, 12):                                  # also when the width of a uniform-row instance is forced
        forced = planner("g4_physical", None, _sw(TPG=tpg))
        assert forced["TPG"] == tpg and forced["uniform45"] == 0 and forced["cg_barriers"] == 4
    # a single LDS vector costs one barrier more; it exists for widths 8 and 12 (640-thread class) only
    sb = planner("g4", None, _sw(SB=1, TPG=8))
    assert sb["sb"] == 1 and sb["uniform45"] == 0 and sb["cg_barriers"] == 4 + 1
    assert sb["instance_name"] == lc.inst(8, False, 1024, True)
    narrow = planner("g4", None, _sw(SB=1))              # the switch alone: the smallest width, which has no such instance
    assert narrow["sb"] == 0 and narrow["uniform45"] == 0 and narrow["cg_barriers"] == 4


# ------------------------------------------------------------------------------------------------ no plan
def test_graphs_without_a_plan(planner):
    """N = 1100, T = 24: more than 1024 threads at every width.  N = 1024, T = 12 as a generic instance
    (MGADMM_LDS_RAGGED): two vectors of 1024 x 12 floats and all tables exceed 160 KiB; the uniform-row instance of the
    same graph, which keeps only the tail table in LDS, fits."""
    wide = planner("n1100", lambda: _uniform_product(1100, 24), {})
    big = planner("n1024", lambda: _uniform_product(1024, 12), _sw(RAGGED=1))
    for p in (wide, big):
        assert p["status"] == NO_PLAN and p["ok"] == 0 and p["image_ints"] == 0 and p["instance"] == -1 and p["cg_barriers"] == 0
        assert all(p[k] == 0 for k in ("TPG", "G", "nthreads", "block", "NR", "lds_bytes", "csr_ints"))
    fits = planner("n1024", None, {})
    assert fits["ok"] == 1 and fits["instance_name"] == lc.uni(12, 1024, False, 1)


# ------------------------------------------------------------------------------------------------ byte identity
@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(GOLDEN, "lds_plan_parent.json")) as f:
        return json.load(f)["cases"]


def test_the_recorded_cases_are_these(parent):
    assert sorted(parent) == sorted(CASES)


@pytest.fixture(scope="module")
def planned(planner):
    """Every case of CASES planned, eight at a time (the graph files are written first, one after the other)."""
    for key, build, _ in CASES.values():
        planner(key, build, _sw(BANK_SEARCH=0))
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        return dict(zip(CASES, pool.map(lambda c: planner(*c), CASES.values())))


@pytest.mark.parametrize("name", list(CASES))
def test_plan_and_image_equal_the_parent_commit(planned, parent, name):
    p = planned[name]
    assert parent[name]["switches"] == CASES[name][2]
    assert parent[name]["ok"] == 1 and len(parent[name]) == len(PLAN_FIELDS) + 1
    for k in PLAN_FIELDS:
        assert p[k] == parent[name][k], (name, k, p[k], parent[name][k])
