"""CPU checks of per-sample graph weights (mgadmm_solver_set_sample_graphs, solve(graph_params=...) / solve(graph_sets=...),
sweep with sigma keys).  None of it needs a GPU.

  * tests/cpu/lds_graph_sets_check.cpp (AddressSanitizer + UBSan, a program of its own) on five graphs -- four census rows
    (uniform rows with a compile-time tail of 2 pairs, uniform rows with a run-time tail, a generic instance with ragged rows,
    a single-buffer instance) and cfg2 -- with four weight sets each: the image of set j inside the table equals, byte for
    byte, what ldsplan::make returns for set j alone; plan and node_of_row equal set 0's; a set with an entry dropped, with
    another k, or under the other transpose rule is refused with the name of what differs.  The property does not depend on
    the length of the bank search (fixed seeds, column offsets only): the program runs 13 plans per graph, which under the
    sanitizers takes minutes at the default 4000 steps, so the graphs are planned at SEARCH steps, side by side;
  * the header's declaration, the ctypes mirror and the exported symbol;
  * validation of graph_params / graph_sets before the library is touched;
  * sweep() forming its cells with sigma keys;
  * the table helper factored out of the constructor: the constructor's u_ew / d_ew of the g1 fixtures, bit for bit."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests"))

import lds_census as lc                       # noqa: E402
import test_lds_plan_cpu as tp                # noqa: E402

SEARCH = 200
PLAN_FIELDS = ("instance", "tail_pairs", "off_lead_t", "off_tail_t", "off_diag", "off_node", "off_rown", "lds_img0", "lds_img_ints",
               "csr_ints", "lds_bytes", "npos", "nthreads", "NR", "TS", "slots", "uniform45")
IMAGE_PARTS = ("rp_u", "rp_d", "en_u", "en_d", "lead_t", "tail_t", "node_of_row", "row_of_node")


def _row(expect):
    return next(r for r in lc.CENSUS if r["expect"] == expect)


GRAPHS = {
    "uniform_tp2": (lambda: tp._census_product(_row(lc.uni(8, 1024, True, 2))), _row(lc.uni(8, 1024, True, 2))["env"]),
    "uniform_runtime_tail": (lambda: tp._census_product(_row(lc.uni(8, 1024, True, -1))), {}),
    "generic_ragged": (lambda: tp._census_product(_row(lc.inst(3, False, 1024, False))), {}),
    "single_buffer": (lambda: tp._census_product(_row(lc.inst(12, False, 640, True))), _row(lc.inst(12, False, 640, True))["env"]),
    "cfg2": (lambda: tp._bench_product("cfg2"), {}),
}


@pytest.fixture(scope="module")
def checked(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("graph_sets")
    exe = str(tmp / "lds_graph_sets_check")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-pthread", "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "cpu", "lds_graph_sets_check.cpp"), "-o", exe])
    jobs = []
    for name, (build, switches) in GRAPHS.items():
        path = str(tmp / (name + ".graph"))
        tp.write_graph(tp.planner_input(build()), path)
        sw = dict(switches, MGADMM_LDS_BANK_SEARCH=str(SEARCH))
        jobs.append((name, [exe, path] + [f"{k}={v}" for k, v in sorted(sw.items())]))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MGADMM_LDS_")}

    def run(job):
        out = subprocess.run(job[1], capture_output=True, text=True, env=env)
        assert out.returncode == 0, (job[0], out.stdout + out.stderr)
        return json.loads(out.stdout)
    with ThreadPoolExecutor(min(len(jobs), os.cpu_count() or 1)) as pool:
        return dict(zip([j[0] for j in jobs], pool.map(run, jobs)))


@pytest.mark.parametrize("name", list(GRAPHS))
def test_images_of_a_table_equal_the_sets_planned_alone(checked, name):
    """Exit status 0 of the program is the byte comparison; here: it ran on the intended instance and named the refusals."""
    from mgadmm import _lib
    out = checked[name]
    assert out["sets"] == 4 and out["img_stride"] % 4 == 0 and 0 <= out["img_stride"] - out["csr_ints"] < 4
    want = {"uniform_tp2": lc.uni(8, 1024, True, 2), "uniform_runtime_tail": lc.uni(8, 1024, True, -1),
            "generic_ragged": lc.inst(3, False, 1024, False), "single_buffer": lc.inst(12, False, 640, True)}
    if name in want:
        assert _lib.decode_lds_instance(out["instance"]) == want[name]
    else:
        assert out["uniform45"] == 1 and _lib.decode_lds_instance(out["instance"]).startswith("k_admm_lds<8, false, 1024, false, 4, 5, true,")
    for k in ("dropped", "other_k", "other_transpose"):
        assert out[k] in PLAN_FIELDS + IMAGE_PARTS, (k, out[k])
    if out["uniform45"]:
        # a uniform-row instance needs 4 + 5 entries in every row and the exact transpose: each of the three loses it
        assert (out["dropped"], out["other_k"], out["other_transpose"]) == ("instance",) * 3
    else:
        assert out["dropped"] == "off_lead_t" and out["other_k"] in ("tail_pairs", "off_en_d", "off_lead_t")      # fewer entries: tables move
        assert out["other_transpose"] in ("tail_pairs", "lead_t", "tail_t", "npos")


# ------------------------------------------------------------------------------------------------ ABI
def test_header_binding_and_symbol_agree():
    from mgadmm import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgadmm.h")).read(), flags=re.S)
    assert re.search(r"int mgadmm_solver_set_sample_graphs\(mgadmm_solver\* s, int32_t n_sets, mgadmm_graph\* const\* graphs, "
                     r"const int32_t\* set_of_sample,\s*int32_t B\);", txt)
    res, args = _lib.SYMBOLS["mgadmm_solver_set_sample_graphs"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32]
    assert _lib.lib.mgadmm_solver_set_sample_graphs.argtypes == args
    assert _lib.lib.mgadmm_solver_set_sample_graphs(None, 0, None, None, 0) == _lib.ERR_INVALID
    assert b"set_sample_graphs" in _lib.lib.mgadmm_last_error()
    m = re.match(r"mgadmm 0\.3\.(\d+) ", _lib.version())
    assert m and int(m.group(1)) >= 2, _lib.version()
    assert "0.3.2: mgadmm_solver_set_sample_graphs" in open(os.path.join(ROOT, "include", "mgadmm.h")).read()
    assert _lib.Params._fields_[-1][0] == "admm_convergence" and _lib.History._fields_[-1][0] == "n_iters_per_sample"      # no struct grew


def test_launch_arguments_grow_behind_what_existing_kernels_read():
    """New LdsArgs fields go behind off_node: no offset that k_admm_lds / k_admm_lds_ps read moves."""
    txt = open(os.path.join(PKG, "csrc", "lds_args.h")).read()
    body = txt[txt.index("struct LdsArgs : LdsArgsCore"):]
    body = re.sub(r"//.*", "", body[:body.index("};")])
    names = re.findall(r"(\w+)(?:\[[^\]]*\])?\s*;", body)
    assert names[-3:] == ["off_node", "img_stride", "gset"], names


# ------------------------------------------------------------------------------------------------ Python validation
def _knn(**kw):
    from mgadmm.ADMM import ADMM_algorithm
    g = load_golden("g1_tables_small.npz")
    cl, dl = torch.from_numpy(g["knn_cl"]).to(torch.int64), torch.from_numpy(g["knn_dl"])
    info = dict(rho=1, rho_u=1, rho_d=1, mu_u=1, mu_d1=1, mu_d2=1)
    return ADMM_algorithm({"n_nodes": int(g["n"])}, info, use_kNN=True, k=int(g["k"]), u_sigma=float(g["sigma"]),
                          d_sigma=float(g["sigma"]), tables=(cl, dl), **kw)


BAD = [
    ({"sigma": [1, 1, 1]}, "unknown key 'sigma'"),
    ({"u_sigma": [1, 1]}, "length B = 3"),
    ({"d_sigma": 2.0}, "length B = 3"),
    ({"u_sigma": [1, float("nan"), 1]}, r"\['u_sigma'\]\[1\] is not finite"),
    ({"d_sigma": np.array([1, 1, np.inf])}, r"\['d_sigma'\]\[2\] is not finite"),
    ({"u_sigma": [1, 0, 1]}, r"\['u_sigma'\]\[1\]"),
    ({"d_sigma": torch.tensor([1.0, 1.0, -2.0])}, r"\['d_sigma'\]\[2\]"),
    ([1, 2, 3], "must be a dict"),
]


@pytest.mark.parametrize("gp, msg", BAD, ids=[m for _, m in BAD])
def test_graph_params_are_validated_before_the_library_is_touched(gp, msg, monkeypatch):
    blk = _knn()
    touched = []
    monkeypatch.setattr(type(blk), "_solver", lambda self, *a: touched.append(a))
    y = torch.ones(3, 12, blk.n_nodes, 1)
    with pytest.raises(ValueError, match=msg):
        blk.solve(y, graph_params=gp)
    with pytest.raises(ValueError, match=msg):
        blk.combined_loop(y, print_info=False, graph_params=gp)
    assert touched == [] and blk._solvers == {}


def test_graph_arguments_refused_for_a_line_graph_and_inconsistent_forms(monkeypatch):
    line = _knn(use_line_graph=True)
    touched = []
    monkeypatch.setattr(type(line), "_solver", lambda self, *a: touched.append(a))
    y = torch.ones(3, 12, line.n_nodes, 1)
    with pytest.raises(ValueError, match="line-graph"):
        line.solve(y, graph_params={"u_sigma": [1.0, 2.0, 3.0]})
    blk = _knn()
    del blk.dist_list
    with pytest.raises(ValueError, match="without distances"):
        blk.solve(y, graph_params={"u_sigma": [1.0, 2.0, 3.0]})
    blk = _knn()
    pair = (blk.u_ew, blk.d_ew)
    for kw, msg in ((dict(graph_of_sample=[0, 0, 0]), "needs graph_sets"),
                    (dict(graph_sets=[pair], graph_params={"u_sigma": [1, 1, 1]}), "exclude each other"),
                    (dict(graph_sets=[pair]), "needs graph_of_sample"),
                    (dict(graph_sets=[], graph_of_sample=[0, 0, 0]), "empty"),
                    (dict(graph_sets=[pair], graph_of_sample=[0, 0]), "B = 3 integers"),
                    (dict(graph_sets=[pair], graph_of_sample=[0, 1, 0]), r"graph_of_sample\[1\] = 1 out of range"),
                    (dict(graph_sets=[pair], graph_of_sample=[0, -1, 0]), "out of range"),
                    (dict(graph_sets=[(blk.u_ew[:, :, :2], blk.d_ew)], graph_of_sample=[0, 0, 0]), "u_ew has shape"),
                    (dict(graph_sets=[blk.u_ew], graph_of_sample=[0, 0, 0]), "must be a pair")):
        with pytest.raises(ValueError, match=msg):
            blk.solve(y, **kw)
    assert touched == []


def test_distinct_pairs_and_the_set_of_every_sample():
    """graph_params -> the distinct (u_sigma, d_sigma) pairs in order of first appearance; a missing key follows the instance."""
    blk = _knn()
    s = blk.u_sigma
    sets, gos = blk._check_graph_sets(None, None, {"u_sigma": [s, 2 * s, s, 2 * s, 3 * s]}, 5)
    assert gos.dtype == np.int32 and gos.tolist() == [0, 1, 0, 1, 2] and len(sets) == 3
    assert torch.equal(sets[0][0], blk.u_ew) and all(torch.equal(d, blk.d_ew) for _, d in sets)
    assert not torch.equal(sets[1][0], blk.u_ew)
    sets, gos = blk._check_graph_sets(None, None, {"u_sigma": [s, s, 2 * s], "d_sigma": [s, 2 * s, 2 * s]}, 3)
    assert gos.tolist() == [0, 1, 2] and torch.equal(sets[0][1], blk.d_ew) and torch.equal(sets[1][1], sets[2][1])
    assert blk._check_graph_sets(None, None, None, 3) is None


# ------------------------------------------------------------------------------------------------ sweep
class _Stub:
    def __init__(self, blk):
        self.blk, self.calls = blk, []

    def __call__(self, y, mask=None, sample_params=None, graph_params=None, **kw):
        self.calls.append(dict(y=y.clone(), sp=sample_params, gp=graph_params, kw=kw))
        B = y.shape[0]
        code = torch.tensor([100 * sample_params["mu_u"][b] + 10 * graph_params["u_sigma"][b] + graph_params["d_sigma"][b] for b in range(B)])
        x = (y[:, :1, :1, :1] * 1000 + code.reshape(B, 1, 1, 1)).expand(B, 24, 2, 1).clone()
        self.blk.n_iters_per_sample = np.arange(B, dtype=np.int32)
        return x, (None, None), None, {}


def test_sweep_forms_its_cells_with_sigma_keys(monkeypatch):
    blk = _knn()
    stub = _Stub(blk)
    monkeypatch.setattr(blk, "solve", stub)
    W = 3
    y = torch.arange(W, dtype=torch.float32).reshape(W, 1, 1, 1).expand(W, 12, 2, 1).clone()
    grid = {"u_sigma": [1, 2], "mu_u": [0.5, 4], "d_sigma": [3, 5]}
    x, n, sets = blk.sweep(y, grid)
    assert sets == [dict(u_sigma=a, mu_u=b, d_sigma=c) for a in (1, 2) for b in (0.5, 4) for c in (3, 5)]      # itertools.product order
    assert tuple(x.shape) == (8, W, 24, 2, 1) and n.shape == (8, W) and n.ravel().tolist() == list(range(8 * W))
    c = stub.calls[0]
    assert len(stub.calls) == 1 and c["kw"] == {"return_state": False}
    assert list(c["sp"]) == ["mu_u"] and list(c["gp"]) == ["u_sigma", "d_sigma"]
    for p, s in enumerate(sets):
        for w in range(W):
            assert float(x[p, w, 0, 0, 0]) == 1000 * w + 100 * s["mu_u"] + 10 * s["u_sigma"] + s["d_sigma"], (p, w)
    # without sigma keys solve() is called as before: no graph argument at all
    stub2 = []
    monkeypatch.setattr(blk, "solve", lambda y, mask=None, sample_params=None, **kw: (
        stub2.append(kw), setattr(blk, "n_iters_per_sample", np.zeros(y.shape[0], np.int32)), (y.expand(y.shape[0], 12, 2, 1).clone(), None, None, {}))[-1])
    blk.sweep(y, {"mu_u": [1, 2]})
    assert stub2 == [{"return_state": False}]
    with pytest.raises(ValueError, match="unknown key"):
        blk.sweep(y, {"k": [4]})


# ------------------------------------------------------------------------------------------------ the table helper
@pytest.mark.parametrize("name", ["small", "pems", "ties", "road400"])
def test_the_table_helper_is_the_constructors_code(name):
    """_weight_tables(u_sigma, d_sigma) is what __init__ runs: the reference's tables of the g1 fixtures bit for bit, for the
    fixture's sigma, the default sigma (None) and both graph kinds; the line graph keeps its sigma-free d_ew."""
    from mgadmm.ADMM import ADMM_algorithm
    g = load_golden(f"g1_tables_{name}.npz")
    n, k, sigma, T = int(g["n"]), int(g["k"]), float(g["sigma"]), 6
    info = dict(rho=1, rho_u=1, rho_d=1, mu_u=1, mu_d1=1, mu_d2=1)
    ue, ud = torch.from_numpy(g["u_edges"]), torch.from_numpy(g["u_dist"])
    tables = (torch.from_numpy(g["knn_cl"]).to(torch.int64), torch.from_numpy(g["knn_dl"]))
    knn = ADMM_algorithm({"n_nodes": n}, info, use_kNN=True, k=k, u_sigma=sigma, d_sigma=sigma, tables=tables, T=T, t_in=3)
    phys = ADMM_algorithm({"n_nodes": n, "u_edges": ue, "u_dist": ud}, info, use_kNN=False, u_sigma=sigma, d_sigma=sigma, T=T, t_in=3)
    for blk, pre in ((knn, "knn"), (phys, "phys")):
        assert blk.u_ew.shape[0] == T and blk.d_ew.shape[0] == T - 1
        np.testing.assert_array_equal(blk.u_ew[0].numpy(), g[pre + "_u_ew"])
        np.testing.assert_array_equal(blk.d_ew[T - 2].numpy(), g[pre + "_d_ew"])
        u, d, tl = blk._weight_tables(sigma, sigma)
        assert tl is None and torch.equal(u, blk.u_ew) and torch.equal(d, blk.d_ew)
        u2, d2, _ = blk._weight_tables(2 * sigma, sigma)
        assert not torch.equal(u2, blk.u_ew) and torch.equal(d2, blk.d_ew)
    u, d, _ = knn._weight_tables(None, None)
    np.testing.assert_array_equal(u[0].numpy(), g["knn_u_ew_defsigma"])
    np.testing.assert_array_equal(d[0].numpy(), g["knn_d_ew_defsigma"])
    flat = ADMM_algorithm({"n_nodes": n}, info, use_kNN=True, k=k, u_sigma=sigma, d_sigma=sigma, tables=tables, T=T, t_in=3,
                          expand_time_dim=False)
    np.testing.assert_array_equal(flat.u_ew.numpy(), g["knn_u_ew"])
    line = ADMM_algorithm({"n_nodes": n}, info, use_kNN=True, k=k, u_sigma=sigma, tables=tables, T=T, t_in=3, use_line_graph=True,
                          skip_connection=2)
    u, d, tl = line._weight_tables(sigma, None)
    assert torch.equal(u, line.u_ew) and torch.equal(d, line.d_ew) and torch.equal(tl, line.time_list)
