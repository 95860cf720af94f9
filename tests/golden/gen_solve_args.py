"""What the Python front end answers to the arguments of a solve, as data: tests/golden/solve_args_parent.json.

    python tests/golden/gen_solve_args.py            # on a checkout of the commit whose answers are to be kept

writes the file (the file in the tree was written on the commit before mgadmm/solve_args.py existed, with this script copied
into a checkout of it; it uses nothing but names importable from mgadmm.ADMM there); tests/test_solve_args_cpu.py imports this
module, forms the same answers with the tree it runs in and compares them with the file, id by id.  Nothing here needs a GPU:
the library is never asked to compute.  The file holds every distinct outcome, ABI call and final state once (`pack`).

  rows    input -> exception type and FULL message, or the normalised result, of the validators called directly
          (_check_sample_params, _check_param_schedule, _check_adaptive_rho, ADMM_algorithm._check_graph_sets, geometric_ramp,
          sweep) and of solve() / combined_loop() driven up to `_solver`, which is replaced by one that raises `Reached`
          (so "Reached" as the type means: every check in front of the library passed);
  traces  solve() / two_loops() / combined_loop() run end to end with `_lib.lib` replaced by a recording stub, `_device` by the
          CPU device and `_stream_ptr` by a null pointer: the sequence of ABI calls -- function, integers, null / non-null of
          every pointer, the fields of every struct, the contents of every host array a setter is given, handles by number --
          then what reached the caller.  For the 12 admissible combinations of sample_params, graph_params, param_schedule and
          adaptive_rho: all calls succeed; every setter in turn refuses; mgadmm_solve refuses / reports non-finite iterates; a
          warm_start that misses a key;
  raise_sites   every `raise` statement of mgadmm/ADMM.py (and mgadmm/solve_args.py where it exists) outside `_device`, found
          with `ast`, against the lines the exceptions above came from: `main` refuses to write a file unless all are hit.
"""
import ast
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(ROOT, "mixed-graph-admm_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)
FIXTURE = os.path.join(HERE, "solve_args_parent.json")
SOURCES = ("ADMM.py", "solve_args.py")
B = 3


class Reached(Exception):
    """raised by the replaced `_solver`: the arguments passed every check in front of the library"""


# ------------------------------------------------------------------------------------------------ raise statements
def raise_sites():
    """{(file, first line, last line)} of the raise statements of the front end, `_device` (no GPU: not an argument) excepted"""
    out = set()
    for name in SOURCES:
        path = os.path.join(PKG, "mgadmm", name)
        if not os.path.exists(path):
            continue

        def walk(node, skip):
            for ch in ast.iter_child_nodes(node):
                sk = skip or (isinstance(ch, ast.FunctionDef) and ch.name == "_device")
                if isinstance(ch, ast.Raise) and not sk:
                    out.add((name, ch.lineno, ch.end_lineno))
                walk(ch, sk)
        walk(ast.parse(open(path).read()), False)
    return out


class Recorder:
    """Outcomes of calls, and the raise statements their exceptions came from."""

    def __init__(self):
        self.sites, self.hit = raise_sites(), set()

    def outcome(self, fn, norm=lambda r: r):
        try:
            res = fn()
        except Exception as e:          # noqa: BLE001 -- the type is part of the answer
            tb, last = e.__traceback__, None
            while tb is not None:
                f = os.path.basename(tb.tb_frame.f_code.co_filename)
                if f in SOURCES and os.path.dirname(tb.tb_frame.f_code.co_filename) == os.path.join(PKG, "mgadmm"):
                    last = (f, tb.tb_lineno)
                tb = tb.tb_next
            if last is not None:
                self.hit |= {s for s in self.sites if s[0] == last[0] and s[1] <= last[1] <= s[2]}
            return {"raises": type(e).__name__, "message": str(e)}
        return {"returns": norm(res)}


# ------------------------------------------------------------------------------------------------ normalised results
def sig6(v):
    """Six significant digits: for values of the float32 weight tables, which `exp` leaves with last bits that depend on the
    CPU's vector units (7.2 digits in the format; any two sigmas of the cases differ in the first two)."""
    return float(f"{v:.6g}")


def n_arrays(d):
    return [[k, str(v.dtype), list(v.shape), bool(v.flags.c_contiguous), v.tolist()] for k, v in d.items()]


def n_schedule(r):
    return {"arrays": n_arrays(r[0]), "K": r[1], "cols": r[2]}


def n_adaptive(r):
    ar, start = r
    return {"every": ar.every, "until": ar.until, "mu": ar.mu, "tau": ar.tau, "rho_min": list(ar.rho_min), "rho_max": list(ar.rho_max),
            "start": start}


def n_graph(r):
    if r is None:
        return None
    sets, gos = r
    return {"n_sets": len(sets), "graph_of_sample": gos.tolist(), "dtype": str(gos.dtype),
            "shapes": [[list(u.shape), list(d.shape)] for u, d in sets], "u_sums": [sig6(float(u.double().sum())) for u, _ in sets]}


# ------------------------------------------------------------------------------------------------ instances
def tiny(**kw):
    from mgadmm.ADMM import ADMM_algorithm
    cl = torch.tensor([[0, 1], [1, 0]])
    return ADMM_algorithm({"n_nodes": 2}, dict(rho=1, rho_u=1, rho_d=1, mu_u=1, mu_d1=1, mu_d2=1), use_kNN=True,
                          u_sigma=1.0, d_sigma=1.0, tables=(cl, torch.tensor([[0.0, 1.0], [0.0, 1.0]])), **kw)


def knn(**kw):
    from mgadmm.ADMM import ADMM_algorithm
    g = np.load(os.path.join(HERE, "g1_tables_small.npz"), allow_pickle=False)
    cl, dl = torch.from_numpy(g["knn_cl"]).to(torch.int64), torch.from_numpy(g["knn_dl"])
    info = dict(rho=1, rho_u=1, rho_d=1, mu_u=1, mu_d1=1, mu_d2=1)
    return ADMM_algorithm({"n_nodes": int(g["n"])}, info, use_kNN=True, k=int(g["k"]), u_sigma=float(g["sigma"]),
                          d_sigma=float(g["sigma"]), tables=(cl, dl), **kw)


ONES = np.ones((4, 3))


def _with(r, b, v):
    a = ONES.copy()
    a[r, b] = v
    return a


# the BAD lists of tests/test_sample_params_cpu.py, test_param_schedule_cpu.py, test_lds_adapt_cpu.py, test_lds_graph_sets_cpu.py
BAD_SP = [{"rho_x": [1, 1, 1]}, {"rho": [1, 1]}, {"mu_u": [[1, 1, 1]]}, {"mu_u": 1.0}, {"rho": [1, 0, 1]},
          {"rho_u": torch.tensor([1.0, 1.0, -2.0])}, {"rho_d": [0.0, 1, 1]}, {"mu_d1": [1, float("nan"), 1]},
          {"mu_d2": np.array([1, 1, np.inf])}, {"mu_u": [1, 1, -1e-9]}, [1, 2, 3]]
GOOD_SP = [{"mu_u": [0, 1, 2], "rho": torch.tensor([1, 2, 3])}, {}, {"rho_d": np.asfortranarray(ONES * 2)[1]},
           {nm: np.full(3, 1.5, dtype=np.float32) for nm in ("mu_d2", "mu_d1", "mu_u", "rho_d", "rho_u", "rho")}]
BAD_SCH = [
    dict(param_schedule={"rho_x": [1, 1]}), dict(param_schedule=[1, 2, 3]), dict(param_schedule={"rho": np.ones((4, 2))}),
    dict(param_schedule={"rho": np.ones((4, 3, 1))}), dict(param_schedule={"rho": 1.0}), dict(param_schedule={"rho": np.ones((0, 3))}),
    dict(param_schedule={"rho": ONES, "mu_u": np.ones((5, 3))}), dict(param_schedule={"rho": ONES, "mu_u": np.ones(4)}),
    dict(param_schedule={"rho": _with(2, 1, 0.0)}), dict(param_schedule={"rho_u": torch.from_numpy(_with(3, 2, -2.0))}),
    dict(param_schedule={"rho_d": [1.0, 1.0, 0.0]}), dict(param_schedule={"mu_d1": _with(0, 0, np.nan)}),
    dict(param_schedule={"mu_d2": [1.0, np.inf]}), dict(param_schedule={"mu_u": _with(1, 2, -1e-9)}),
    dict(param_schedule={"mu_u": ONES}, sample_params={"mu_u": [1, 1, 1]}), dict(param_schedule={"rho": ONES}, schedule_start=-1),
    dict(param_schedule={"rho": ONES}, schedule_start=1.5),
    # order inside the check: not a dict before schedule_start before the entries; the entries in the dict's order; per entry
    # unknown key, given twice, shape, the shape of the entries before, finite, sign
    dict(param_schedule=3.5, schedule_start=-1), dict(param_schedule={"rho_x": [1]}, schedule_start=-1),
    dict(param_schedule={"mu_u": ONES, "rho_x": ONES}, sample_params={"mu_u": [1, 1, 1]}),
    dict(param_schedule={"rho_x": ONES, "mu_u": ONES}, sample_params={"mu_u": [1, 1, 1]}),
    dict(param_schedule={"mu_u": np.ones((4, 2))}, sample_params={"mu_u": [1, 1, 1]}),
    dict(param_schedule={"rho": ONES, "mu_u": np.full((5, 2), np.nan)}), dict(param_schedule={"rho": ONES, "mu_u": np.full(4, np.nan)}),
    dict(param_schedule={"rho": [1.0, -1.0, np.nan, 0.0]}), dict(param_schedule={"mu_u": [-1.0, 1.0], "rho": [0.0, 0.0]}),
    dict(param_schedule={"rho": np.ones(0)}),
]
GOOD_SCH = [
    dict(param_schedule={"mu_u": [0, 1, 2, 3], "rho": torch.tensor([1, 2, 3, 4])}),
    dict(param_schedule={"rho_d": np.asfortranarray(ONES * 2)}, schedule_start=7, sample_params={"rho": np.ones(3)}),
    dict(param_schedule={}), dict(param_schedule={"rho": np.ones((3, 3))}), dict(param_schedule={"rho": [2.0]}, schedule_start=40),
    dict(param_schedule={"mu_d1": np.arange(12.0).reshape(4, 3), "rho_u": ONES + 1}, schedule_start=True),
]
BAD_AR = [
    dict(adaptive_rho=[4, 10, 2]), dict(adaptive_rho={"every": 4, "nu": 2}), dict(adaptive_rho={"mu": 10}), dict(adaptive_rho={"every": 0}),
    dict(adaptive_rho={"every": 17}), dict(adaptive_rho={"every": 4, "mu": 1.0}), dict(adaptive_rho={"every": 4, "tau": 0.5}),
    dict(adaptive_rho={"every": 4, "until": -1}), dict(adaptive_rho={"every": 4, "rho_min": 0.0}),
    dict(adaptive_rho={"every": 4, "rho_min": 2.0, "rho_max": [3, 1, 3]}), dict(adaptive_rho={"every": 4, "rho_max": [1, 2]}),
    dict(adaptive_rho={"every": 4, "rho_max": {"mu_u": 1}}), dict(adaptive_rho={"every": 4}, adaptive_start=6),
    dict(adaptive_rho={"every": 4}, adaptive_start=-4),
    # order inside the check
    dict(adaptive_rho={"every": None, "nu": 1}), dict(adaptive_rho={"every": 0, "mu": 1.0, "until": -1}),
    dict(adaptive_rho={"every": 4, "mu": 1.0, "until": -1}, adaptive_start=6), dict(adaptive_rho={"every": 4, "until": -1}, adaptive_start=6),
    dict(adaptive_rho={"every": 4, "rho_min": [1, 2]}, adaptive_start=6), dict(adaptive_rho={"every": 4, "rho_max": float("inf")}),
    dict(adaptive_rho={"every": 4, "rho_min": {"rho_d": 9.0}, "rho_max": 4.0}),
]
GOOD_AR = [
    dict(adaptive_rho={"every": 4}, adaptive_start=8),
    dict(adaptive_rho={"every": 2, "mu": 3, "tau": 1.5, "until": 12, "rho_min": {"rho_u": 0.5}, "rho_max": [4, 5, 6]}),
    dict(adaptive_rho={"every": 16, "until": None, "rho_min": np.float32(0.5), "rho_max": {"rho": 1, "rho_d": 2}}, adaptive_start=True),
]
BAD_GP = [{"sigma": [1, 1, 1]}, {"u_sigma": [1, 1]}, {"d_sigma": 2.0}, {"u_sigma": [1, float("nan"), 1]}, {"d_sigma": np.array([1, 1, np.inf])},
          {"u_sigma": [1, 0, 1]}, {"d_sigma": torch.tensor([1.0, 1.0, -2.0])}, [1, 2, 3], {"u_sigma": [1, -1, np.nan]}]


def graph_cases(blk):
    """keyword sets of the graph arguments on the kNN instance `blk` (B = 3), refused ones and accepted ones"""
    pair, s = (blk.u_ew, blk.d_ew), blk.u_sigma
    return [dict(graph_of_sample=[0, 0, 0]), dict(graph_sets=[pair], graph_params={"u_sigma": [1, 1, 1]}), dict(graph_sets=[pair]),
            dict(graph_sets=[], graph_of_sample=[0, 0, 0]), dict(graph_sets=[pair], graph_of_sample=[0, 0]),
            dict(graph_sets=[pair], graph_of_sample=[0, 1, 0]), dict(graph_sets=[pair], graph_of_sample=[0, -1, 0]),
            dict(graph_sets=[(blk.u_ew[:, :, :2], blk.d_ew)], graph_of_sample=[0, 0, 0]), dict(graph_sets=[blk.u_ew], graph_of_sample=[0, 0, 0]),
            dict(graph_sets=[pair], graph_of_sample=[0.0, 0.0, 0.0]), dict(graph_sets=[pair], graph_of_sample=[[0, 0, 0]]),
            dict(graph_sets=[pair, (blk.u_ew, blk.d_ew[:1])], graph_of_sample=[0, 0, 0]),
            dict(graph_sets=[pair, blk.u_ew], graph_of_sample=[5, 5]), dict(graph_sets=[(blk.u_ew[:1], blk.d_ew)]),
            # accepted
            dict(), dict(graph_params={"u_sigma": [s, 2 * s, s]}), dict(graph_params={"u_sigma": [s, s, 2 * s], "d_sigma": [s, 2 * s, 2 * s]}),
            dict(graph_params={}), dict(graph_sets=[pair, (blk.u_ew[0] * 2, blk.d_ew[0])], graph_of_sample=torch.tensor([1, 0, 1])),
            dict(graph_sets=[pair], graph_of_sample=np.zeros(3, dtype=np.uint8))]


# two refusals due at once: the earlier one of the order of refusals is the answer (sample_params, param_schedule, the graph
# arguments, adaptive_rho, adaptive_rho with param_schedule, then y and the mask)
Y3 = torch.ones(B, 12, 2)
PAIRS = [
    ("sample_params+param_schedule", dict(sample_params={"rho": [1, 0, 1]}, param_schedule={"rho_x": [1, 1]})),
    ("sample_params+schedule_start", dict(sample_params=[1], param_schedule={"rho": ONES}, schedule_start=-1)),
    ("param_schedule+graph", dict(param_schedule={"rho": np.ones((4, 2))}, graph_of_sample=[0, 0, 0])),
    ("schedule_start+graph_params", dict(param_schedule={"rho": ONES}, schedule_start=-1, graph_params={"sigma": [1, 1, 1]})),
    ("given_twice+graph", dict(param_schedule={"mu_u": ONES}, sample_params={"mu_u": [1, 1, 1]}, graph_of_sample=[0, 0, 0])),
    ("graph+adaptive_rho", dict(graph_of_sample=[0, 0, 0], adaptive_rho={"every": 0})),
    ("graph_params+adaptive_start", dict(graph_params={"u_sigma": [1, 0, 1]}, adaptive_rho={"every": 4}, adaptive_start=6)),
    ("adaptive_rho+exclude", dict(adaptive_rho={"every": 0}, param_schedule={"rho": [1.0, 2.0]})),
    ("adaptive_start+exclude", dict(adaptive_rho={"every": 4}, adaptive_start=6, param_schedule={"rho": ONES})),
    ("exclude+y", dict(adaptive_rho={"every": 4}, param_schedule={"rho": [1.0, 2.0]}, y=Y3)),
    ("exclude+mask", dict(adaptive_rho={"every": 4}, param_schedule={"rho": [1.0, 2.0]}, y=torch.ones(B, 24, 2, 1), mask=torch.ones(B, 24, 2))),
    ("sample_params+y", dict(sample_params={"rho": [1, 1]}, y=Y3)),
    ("adaptive_rho+y", dict(adaptive_rho={"every": 0}, y=Y3)),
    ("y+mask", dict(y=torch.ones(B, 24, 5, 1), mask=torch.ones(B, 24, 2, 1))),
    ("all five", dict(sample_params={"rho": [1, 0, 1]}, param_schedule={"rho_x": [1, 1]}, graph_of_sample=[0], adaptive_rho={"every": 0}, y=Y3)),
    ("B of a y that is refused later", dict(sample_params={"rho": [1, 1, 1, 1]}, y=torch.ones(4, 12, 7, 1))),
]
# solve()'s own handling of y and mask (B = 3, two nodes, t_in = 12, T = 24)
OWN = [
    ("y 3 dims", dict(y=Y3)), ("y nodes", dict(y=torch.ones(B, 12, 5, 1))), ("y steps", dict(y=torch.ones(B, 11, 2, 1))),
    ("y steps with mask", dict(y=torch.ones(B, 12, 2, 1), mask=torch.ones(B, 12, 2, 1))),
    ("mask shape", dict(y=torch.ones(B, 24, 2, 1), mask=torch.ones(B, 24, 2, 2))), ("mask dims", dict(y=torch.ones(B, 24, 2, 1), mask=torch.ones(B, 24, 2))),
    ("accepted", dict(y=torch.ones(B, 12, 2, 1))), ("accepted with mask", dict(y=torch.ones(B, 24, 2, 1), mask=torch.ones(B, 24, 2, 1))),
    ("accepted float64", dict(y=torch.ones(B, 12, 2, 2, dtype=torch.float64))),
]
SWEEP = [
    ("unknown schedule key", dict(grid={}, schedules={"u_sigma": [np.ones(3)]})), ("twice", dict(grid={"rho": [1, 2]}, schedules={"rho": [np.ones(3)]})),
    ("lengths", dict(grid={}, schedules={"rho": [np.ones(3), np.ones(4)]})), ("2-D", dict(grid={}, schedules={"rho": [np.ones((3, 2))]})),
    ("empty candidate", dict(grid={}, schedules={"rho": [torch.ones(0)]})), ("unknown key", dict(grid={"sigma": [1]})),
    ("chunk", dict(grid={"mu_u": [0.5, 1, 2], "mu_d1": [1, 2]}, chunk=0)),
    ("schedule key before grid key", dict(grid={"k": [4]}, schedules={"k": [np.ones(3)]})),
    ("candidate shapes before grid key", dict(grid={"k": [4]}, schedules={"rho": [np.ones(3), np.ones(4)]})),
    ("grid key before chunk", dict(grid={"k": [4]}, chunk=0)),
    ("accepted", dict(grid={"mu_d1": [0.5, 4], "u_sigma": [1, 2]}, schedules={"rho": [torch.tensor([1.0, 2.0]), [3, 4]]}, chunk=5)),
]
RAMP = [(2.0, 1.5, 5), (2.0, 1.5, 5, 5), (0.0, 1.1, 3), (1.0, -1.0, 3), (1.0, 1.1, 0), (float("nan"), 1.1, 3), (1.0, 1.1, 2.5), (1.0, 2.0, 1)]


def _solver_reached(self, *a):
    raise Reached()


def rows(rec, mp):
    import mgadmm.ADMM as A
    out = {}
    mp.setattr(A, "_device", lambda device=None: torch.device("cpu"))
    mp.setattr(A.ADMM_algorithm, "_solver", _solver_reached)
    y = torch.ones(B, 12, 2, 1)

    def via_solve(tag, blk, kw, loop=True):
        kw = dict(kw)
        yy, mask = kw.pop("y", torch.ones(B, 12, blk.n_nodes, 1)), kw.pop("mask", None)
        out[tag + " solve"] = rec.outcome(lambda: blk.solve(yy, mask=mask, **kw))
        if loop and "schedule_start" not in kw and "adaptive_start" not in kw:
            out[tag + " combined_loop"] = rec.outcome(lambda: blk.combined_loop(yy, mask=mask, print_info=False, **kw))
        assert blk._solvers == {} and blk._graphs == {}

    for i, sp in enumerate(BAD_SP + GOOD_SP):
        out[f"sample_params {i}"] = rec.outcome(lambda: A._check_sample_params(sp, B), n_arrays)
        via_solve(f"sample_params {i}", tiny(), dict(sample_params=sp))
    for i, kw in enumerate(BAD_SCH + GOOD_SCH):
        out[f"param_schedule {i}"] = rec.outcome(lambda: A._check_param_schedule(kw["param_schedule"], B, kw.get("schedule_start", 0),
                                                                                   kw.get("sample_params")), n_schedule)
        via_solve(f"param_schedule {i}", tiny(), kw)
    for i, kw in enumerate(BAD_AR + GOOD_AR):
        out[f"adaptive_rho {i}"] = rec.outcome(lambda: A._check_adaptive_rho(kw["adaptive_rho"], kw.get("adaptive_start", 0)), n_adaptive)
        via_solve(f"adaptive_rho {i}", tiny(), kw)
    out["adaptive_rho default start"] = rec.outcome(lambda: A._check_adaptive_rho({"every": 3}), n_adaptive)
    for i, gp in enumerate(BAD_GP):
        blk = knn()
        out[f"graph_params {i}"] = rec.outcome(lambda: blk._check_graph_sets(None, None, gp, B), n_graph)
        via_solve(f"graph_params {i}", blk, dict(graph_params=gp))
    for i, kw in enumerate(graph_cases(knn())):
        blk = knn()
        out[f"graph {i}"] = rec.outcome(lambda: blk._check_graph_sets(kw.get("graph_sets"), kw.get("graph_of_sample"), kw.get("graph_params"), B),
                                        n_graph)
        via_solve(f"graph {i}", blk, kw)
    s5 = knn().u_sigma
    out["graph_params five"] = rec.outcome(lambda: knn()._check_graph_sets(None, None, {"u_sigma": [s5, 2 * s5, s5, 2 * s5, 3 * s5]}, 5), n_graph)
    line = knn(use_line_graph=True)
    for tag, kw in (("line graph_params", dict(graph_params={"u_sigma": [1.0, 2.0, 3.0]})), ("line graph_sets", dict(graph_sets=[], graph_of_sample=[0])),
                    ("line both", dict(graph_sets=[], graph_params=[1])), ("line bad graph_params", dict(graph_params={"sigma": 1})),
                    ("line graph_of_sample alone", dict(graph_of_sample=[0, 0, 0])), ("line none", dict())):
        via_solve(tag, line, kw)
    nodist = knn()
    del nodist.dist_list
    via_solve("no dist_list", nodist, dict(graph_params={"u_sigma": [1.0, 2.0, 3.0]}))
    via_solve("no dist_list, bad key", nodist, dict(graph_params={"sigma": [1.0, 2.0, 3.0]}))
    via_solve("no dist_list, graph_sets", nodist, dict(graph_sets=[(nodist.u_ew, nodist.d_ew)], graph_of_sample=[0, 0, 0]))
    for tag, kw in PAIRS:
        via_solve("pair " + tag, tiny(), kw)
    for tag, kw in OWN:
        via_solve("own " + tag, tiny(), kw, loop=False)
    via_solve("own dtype", tiny(compute_dtype="match"), dict(y=torch.ones(B, 12, 2, 1, dtype=torch.int32)), loop=False)
    via_solve("own dtype match", tiny(compute_dtype="match"), dict(y=torch.ones(B, 12, 2, 1, dtype=torch.float64)), loop=False)
    out["own two_loops mask shape"] = rec.outcome(lambda: tiny().two_loops(torch.ones(B, 24, 2, 1), torch.ones(B, 24, 2, 2)))
    out["own two_loops y steps"] = rec.outcome(lambda: tiny().two_loops(torch.ones(B, 24, 2, 1)))
    out["own two_loops accepted"] = rec.outcome(lambda: tiny().two_loops(y))

    class Solve:               # sweep() up to its solve() calls: what it asks for
        def __init__(self, blk):
            self.blk, self.calls = blk, []

        def __call__(self, y, mask=None, sample_params=None, **kw):
            d = lambda v: {k: np.asarray(a).tolist() for k, a in v.items()} if hasattr(v, "items") else v
            self.calls.append(dict(B=y.shape[0], sample_params=d(sample_params), **{k: d(v) for k, v in kw.items()}))
            self.blk.n_iters_per_sample = np.arange(y.shape[0], dtype=np.int32)
            return y[:, :1].expand(y.shape[0], 24, 2, 1).clone(), (None, None), None, {}
    for tag, kw in SWEEP:
        blk = tiny()
        blk.solve = Solve(blk)
        out["sweep " + tag] = rec.outcome(lambda: blk.sweep(y[:2], **kw), lambda r: dict(
            shape=list(r[0].shape), n=r[1].tolist(), sets=[{k: np.asarray(v).tolist() for k, v in s.items()} for s in r[2]], calls=blk.solve.calls))
    for i, a in enumerate(RAMP):
        out[f"geometric_ramp {i}"] = rec.outcome(lambda: A.geometric_ramp(*a), lambda v: [str(v.dtype), v.tolist()])
    for i, kw in enumerate((dict(cg_convergence="x"), dict(admm_convergence="x"), dict(graph_backend="x"))):
        out[f"constructor {i}"] = rec.outcome(lambda: tiny(**kw), lambda r: None)
    blk = tiny()
    out["CG_solver foreign operator"] = rec.outcome(lambda: blk.CG_solver(tiny().LHS_x, y))
    out["CG_solver plain function"] = rec.outcome(lambda: blk.CG_solver(lambda x: x, y))
    return out


# ------------------------------------------------------------------------------------------------ the recording stub
class StubLib:
    """Stands in for `_lib.lib`: records every call and answers OK, except the `fail[name] = (i, rc)`-th call of `name`."""
    HANDLE = 0x1000

    def __init__(self, fail=None):
        self.calls, self.fail, self.count, self.handles, self.last = [], dict(fail or {}), {}, 0, "nothing"

    def __getattr__(self, name):
        if not name.startswith("mgadmm_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _label(self, v):
        if not v:
            return None
        return f"handle{v // self.HANDLE}" if v % self.HANDLE == 0 and v // self.HANDLE <= self.handles else "ptr"

    def _describe(self, a):
        if a is None or isinstance(a, (bool, int, float)):
            return a
        if hasattr(a, "_obj"):                     # byref(...)
            return self._describe(a._obj)
        if isinstance(a, C.c_void_p):
            return self._label(a.value)
        if isinstance(a, C.Structure):
            out = {}
            for nm, tp in a._fields_:
                v = getattr(a, nm)
                if tp is C.c_void_p:
                    out[nm] = self._label(v)
                elif issubclass(tp, C._Pointer):
                    out[nm] = "ptr" if v else None
                elif issubclass(tp, C.Array):
                    out[nm] = list(v)
                else:
                    out[nm] = v
            return out
        if isinstance(a, C._Pointer):
            return "ptr" if a else None
        if isinstance(a, C.Array):
            return [self._label(v) if a._type_ is C.c_void_p else v for v in a]
        return a.value                             # c_int32 and the like

    @staticmethod
    def _host_arrays(name, args):
        """the contents of the host arrays a call is given, by the lengths its integers state"""
        take = lambda p, n: p[:n] if p else None
        if name == "mgadmm_solver_set_sample_params" and args[1] is not None:
            return {nm: take(getattr(args[1]._obj, nm), args[2]) for nm, _ in args[1]._obj._fields_}
        if name == "mgadmm_solver_set_param_schedule" and args[1] is not None:
            return {nm: take(getattr(args[1]._obj, nm), args[2] * max(args[3], 1)) for nm, _ in args[1]._obj._fields_}
        if name == "mgadmm_solver_set_sample_graphs" and args[3] is not None:
            return {"set_of_sample": take(args[3], args[4])}
        if name == "mgadmm_graph_create":
            d = args[0]._obj
            nu = d.u_rowptr[d.n_nodes]
            out = {"u_rowptr": d.u_rowptr[:d.n_nodes + 1], "u_col": d.u_col[:nu], "u_val": [sig6(v) for v in d.u_val[:nu]]}
            if d.d_rowptr:
                nd = d.d_rowptr[d.n_nodes]
                out.update(d_rowptr=d.d_rowptr[:d.n_nodes + 1], d_col=d.d_col[:nd], d_val=[sig6(v) for v in d.d_val[:nd]])
            if d.band_w:
                out["band_w"] = [sig6(v) for v in d.band_w[:d.T * d.skip]]
            return out
        return None

    def _call(self, name, args):
        if name == "mgadmm_last_error":
            return f"stub: {self.last} refused".encode()
        entry = [name] + [self._describe(a) for a in args]
        arrays = self._host_arrays(name, args)
        if arrays is not None:
            entry.append(arrays)
        self.calls.append(entry)
        i = self.count.get(name, 0)
        self.count[name] = i + 1
        if name in self.fail and self.fail[name][0] == i:
            self.last = name
            return self.fail[name][1]
        if name in ("mgadmm_graph_create", "mgadmm_solver_create"):
            self.handles += 1
            args[-1]._obj.value = self.handles * self.HANDLE
        if name in ("mgadmm_solve", "mgadmm_solve_from"):           # two iterations ran, of three allowed
            args[-2]._obj.n_iters = 2
        if name == "mgadmm_solver_get_adaptive_history":             # two periods; sample b of the second one: 10 f + b + 0.5
            args[4]._obj.value = 2
            if args[2]:
                for j in range(2 * 3 * args[1]):
                    args[2][j] = float(j // (3 * args[1]) * 0.5 + 10 * (j // args[1] % 3) + j % args[1])
        return 0


ARGS = {
    "sample_params": dict(sample_params={"rho": [1, 2, 3], "mu_u": torch.tensor([0.0, 1.0, 2.0])}),
    "graph_params": dict(graph_params={"u_sigma": [1.0, 2.0, 1.0]}),
    "param_schedule": dict(param_schedule={"rho_u": ONES * np.arange(1.0, 5.0)[:, None], "mu_d1": np.arange(12.0).reshape(4, 3)}, schedule_start=1),
    "adaptive_rho": dict(adaptive_rho={"every": 2, "rho_max": [4, 5, 6]}, adaptive_start=2),
}
SETTER = {"sample_params": "mgadmm_solver_set_sample_params", "graph_params": "mgadmm_solver_set_sample_graphs",
          "param_schedule": "mgadmm_solver_set_param_schedule", "adaptive_rho": "mgadmm_solver_set_adaptive_rho"}
COMBOS = [c for n in range(5) for c in itertools.combinations(ARGS, n) if not ("param_schedule" in c and "adaptive_rho" in c)]
assert len(COMBOS) == 12
UNSUPPORTED, NONFINITE = -4, -3


def _summary(blk, res):
    lens = {k: (len(v) if isinstance(v, list) else None if v is None else np.asarray(v).tolist()) for k, v in blk.history().items() if k != "res_name"}
    out = {"history": lens, "state": sorted(getattr(blk, "state", {})),
           "rho_history": None if blk.rho_history is None else blk.rho_history.tolist(),
           "rho_final": None if blk.rho_final is None else blk.rho_final.tolist(),
           "metrics_per_sample": list(blk.metrics_per_sample.shape) if hasattr(blk, "metrics_per_sample") else None}
    if isinstance(res, tuple):
        x, (zu, zd), phi, hist = res
        out["returns"] = dict(x=[list(x.shape), str(x.dtype)], zu=zu is not None, zd=zd is not None, phi=phi is not None, history=sorted(hist))
    elif res is not None:
        out["returns"] = [list(res.shape), str(res.dtype)]
    return out


def trace(rec, mp, run, fail=None, **ctor):
    """one instance on a fresh stub: `run(blk)`, then close(); the calls, what reached the caller, what the instance holds"""
    import mgadmm.ADMM as A
    from mgadmm import _lib
    stub = StubLib(fail)
    mp.setattr(_lib, "lib", stub)
    mp.setattr(A, "_device", lambda device=None: torch.device("cpu"))
    mp.setattr(A, "_stream_ptr", lambda dev: C.c_void_p(None))
    blk = tiny(**ctor)
    blk.max_ADMM_iter, blk.max_CG_iter, blk.max_inner_iter = 3, 4, 2
    res = []
    out = rec.outcome(lambda: res.append(run(blk)), lambda r: None)
    out["after"] = _summary(blk, res[0] if res else None)
    blk.close()
    out["calls"] = stub.calls
    return out


def traces(rec, mp):
    out = {}
    y = torch.ones(B, 12, 2, 1)
    state = lambda: {k: torch.ones(B, 24, 2, 1) for k in ("x", "zu", "zd", "phi", "gamma", "gamma_u", "gamma_d")}
    for combo in COMBOS:
        kw = {}
        for nm in combo:
            kw.update(ARGS[nm])
        tag = "+".join(combo) or "plain"
        solve = lambda blk: blk.solve(y, **kw)
        out[f"{tag}: ok"] = trace(rec, mp, solve)
        for nm in combo:
            out[f"{tag}: {nm} refused"] = trace(rec, mp, solve, {SETTER[nm]: (0, UNSUPPORTED)})
        out[f"{tag}: solve refused"] = trace(rec, mp, solve, {"mgadmm_solve": (0, UNSUPPORTED)})
        out[f"{tag}: non-finite"] = trace(rec, mp, solve, {"mgadmm_solve": (0, NONFINITE)})
        ws = state()
        del ws["gamma_u"]
        out[f"{tag}: warm_start misses a key"] = trace(rec, mp, lambda blk: blk.solve(y, warm_start=ws, **kw))
        out[f"{tag}: warm_start"] = trace(rec, mp, lambda blk: blk.solve(y, warm_start=state(), **kw))
        out[f"{tag}: two solves"] = trace(rec, mp, lambda blk: (blk.solve(y, **kw), blk.solve(y))[1])
    allfour = dict(ARGS["sample_params"], **ARGS["graph_params"], **ARGS["param_schedule"])
    bad_ws = dict(state(), zd=torch.ones(B, 24, 2, 2))
    out["warm_start shape"] = trace(rec, mp, lambda blk: blk.solve(y, warm_start=bad_ws, **allfour))
    out["warm_start of None entries"] = trace(rec, mp, lambda blk: blk.solve(y, warm_start=dict(state(), x=None, phi=None), **ARGS["adaptive_rho"]))
    out["warm_start key and a setter refusing"] = trace(rec, mp, lambda blk: blk.solve(y, warm_start={}, **allfour),
                                                        {SETTER["param_schedule"]: (0, UNSUPPORTED)})
    out["warm_start shape and non-finite"] = trace(rec, mp, lambda blk: blk.solve(y, warm_start=state(), **allfour), {"mgadmm_solve_from": (0, NONFINITE)})
    for abl in ("DGTV", "DGLR", "UT"):
        out[f"ablation {abl}"] = trace(rec, mp, lambda blk: blk.solve(y), ablation=abl)
        out[f"ablation {abl}: warm_start"] = trace(rec, mp, lambda blk: blk.solve(y, warm_start=state()), ablation=abl)
        out[f"ablation {abl}: warm_start of x alone"] = trace(rec, mp, lambda blk: blk.solve(y, warm_start={"x": y}), ablation=abl)
        out[f"ablation {abl}: two_loops"] = trace(rec, mp, lambda blk: blk.two_loops(y), ablation=abl)
    ym, m = torch.ones(B, 24, 2, 1), torch.ones(B, 24, 2, 1, dtype=torch.float64)
    out["mask"] = trace(rec, mp, lambda blk: blk.solve(ym, mask=m))
    out["mask float32, differential"] = trace(rec, mp, lambda blk: blk.solve(y, differential=True) and blk.solve(ym, mask=m.float()))
    out["no state"] = trace(rec, mp, lambda blk: blk.solve(y, return_state=False, **ARGS["adaptive_rho"]))
    out["per-sample history"] = trace(rec, mp, lambda blk: blk.solve(y, per_sample_history=True))
    out["per-sample history: non-finite"] = trace(rec, mp, lambda blk: blk.solve(y, per_sample_history=True), {"mgadmm_solve": (0, NONFINITE)})
    out["adaptive_rho: non-finite"] = trace(rec, mp, lambda blk: blk.solve(y, **ARGS["adaptive_rho"]), {"mgadmm_solve": (0, NONFINITE)})
    out["per-sample stop, no coefficients"] = trace(rec, mp, lambda blk: setattr(blk, "record_cg_coeffs", False) or blk.solve(y),
                                                    admm_convergence="per_sample")
    out["float64, two channels, B = 1"] = trace(rec, mp, lambda blk: blk.solve(torch.ones(1, 12, 2, 2)), compute_dtype=torch.float64)
    out["a larger batch after a smaller one"] = trace(rec, mp, lambda blk: (blk.solve(y[:1]), blk.solve(y, **ARGS["sample_params"]))[1])
    out["admm_convergence changed afterwards"] = trace(rec, mp, lambda blk: setattr(blk, "admm_convergence", "x") or blk.solve(y, **allfour))

    def varying(blk):
        blk.u_ew = blk.u_ew * torch.arange(1.0, 25.0).reshape(24, 1, 1)
        return blk.solve(y, **ARGS["sample_params"])
    out["u_ew varies over time"] = trace(rec, mp, varying)
    # the graph table: the low-level form; a graph that cannot be created midway; the clear call in front of the closes
    def sets(blk):
        return dict(graph_sets=[(blk.u_ew, blk.d_ew), (blk.u_ew[0] * 2, blk.d_ew[0] * 3), (blk.u_ew, blk.d_ew)], graph_of_sample=[2, 0, 1])
    out["graph_sets"] = trace(rec, mp, lambda blk: blk.solve(y, **sets(blk)))
    out["graph_sets: the second graph fails"] = trace(rec, mp, lambda blk: blk.solve(y, **sets(blk), **ARGS["sample_params"]),
                                                      {"mgadmm_graph_create": (2, UNSUPPORTED)})
    out["graph_sets: the first graph fails"] = trace(rec, mp, lambda blk: blk.solve(y, **sets(blk)), {"mgadmm_graph_create": (1, UNSUPPORTED)})
    out["the instance's graph fails"] = trace(rec, mp, lambda blk: blk.solve(y, **allfour), {"mgadmm_graph_create": (0, UNSUPPORTED)})
    out["solver_create fails"] = trace(rec, mp, lambda blk: blk.solve(y, **allfour), {"mgadmm_solver_create": (0, -5)})
    out["line graph"] = trace(rec, mp, lambda blk: blk.solve(y, **ARGS["sample_params"]), use_line_graph=True, skip_connection=2)
    # two_loops and combined_loop
    out["two_loops"] = trace(rec, mp, lambda blk: blk.two_loops(y))
    out["two_loops: mask"] = trace(rec, mp, lambda blk: blk.two_loops(ym, m.float(), differential=False))
    out["two_loops: non-finite"] = trace(rec, mp, lambda blk: blk.two_loops(y), {"mgadmm_two_loops": (0, NONFINITE)})
    out["two_loops: refused"] = trace(rec, mp, lambda blk: blk.two_loops(y), {"mgadmm_two_loops": (0, UNSUPPORTED)})
    out["two_loops: B = 1, DGLR"] = trace(rec, mp, lambda blk: blk.two_loops(y[:1]), ablation="DGLR")
    out["combined_loop"] = trace(rec, mp, lambda blk: blk.combined_loop(y, print_info=False))
    out["combined_loop: mask"] = trace(rec, mp, lambda blk: blk.combined_loop(ym, m, False, False))
    for nm in ARGS:
        kw = {k: v for k, v in ARGS[nm].items() if not k.endswith("_start")}
        out[f"combined_loop: {nm}"] = trace(rec, mp, lambda blk: blk.combined_loop(y, print_info=False, **kw))
    out["combined_loop: graph_sets"] = trace(rec, mp, lambda blk: blk.combined_loop(y, print_info=False, **sets(blk)))
    for k in ("schedule_start", "adaptive_start", "warm_start", "return_state", "per_sample_history"):      # not combined_loop's: solve's TypeError
        out[f"combined_loop: {k}"] = trace(rec, mp, lambda blk: blk.combined_loop(y, print_info=False, **{k: 0}))
    return out


def collect(mp):
    """{"rows", "traces", "raise_sites"} of the tree this module is imported in"""
    rec = Recorder()
    out = {"rows": rows(rec, mp)}
    mp.undo()
    out["traces"] = traces(rec, mp)
    mp.undo()
    out["raise_sites"] = {"total": len(rec.sites), "hit": len(rec.hit), "missed": sorted(f"{f}:{a}" for f, a, _ in rec.sites - rec.hit)}
    return json.loads(json.dumps(out))           # tuples -> lists, as the file holds them


def pack(out):
    """The file's form: every distinct outcome, ABI call and final state once, one per line; rows and traces refer to them by number."""
    tables = {k: [] for k in ("outcomes", "calls", "after")}

    def ref(k, v):
        if v not in tables[k]:
            tables[k].append(v)
        return tables[k].index(v)
    rows = {k: ref("outcomes", v) for k, v in out["rows"].items()}
    traces = {k: [ref("outcomes", {a: b for a, b in t.items() if a not in ("after", "calls")}), ref("after", t["after"]),
                  [ref("calls", c) for c in t["calls"]]] for k, t in out["traces"].items()}
    return dict(raise_sites=out["raise_sites"], **tables, rows=rows, traces=traces)


def unpack(d):
    """`pack` undone: what `collect` returned on the commit the file was written on."""
    traces = {k: dict(d["outcomes"][o], after=d["after"][a], calls=[d["calls"][c] for c in cs]) for k, (o, a, cs) in d["traces"].items()}
    return dict(rows={k: d["outcomes"][o] for k, o in d["rows"].items()}, traces=traces, raise_sites=d["raise_sites"])


def load():
    with open(FIXTURE) as f:
        return unpack(json.load(f))


def main():
    out = collect(pytest.MonkeyPatch())
    sites = out["raise_sites"]
    assert not sites["missed"], sites
    out["raise_sites"] = {"total": sites["total"], "hit": sites["hit"]}
    packed = pack(out)
    assert unpack(json.loads(json.dumps(packed))) == out
    one = lambda v: json.dumps(v, separators=(",", ":"))
    with open(FIXTURE, "w") as f:
        f.write("{" + ",\n".join(
            f'"{k}":' + (one(v) if k == "raise_sites" else
                         "[\n" + ",\n".join(one(e) for e in v) + "\n]" if isinstance(v, list) else
                         "{\n" + ",\n".join(f"{one(a)}:{one(b)}" for a, b in v.items()) + "\n}") for k, v in packed.items()) + "}\n")
    assert load() == out
    refused = sum("raises" in r for r in out["rows"].values())
    print(f"{len(out['rows'])} rows ({refused} refused), {len(out['traces'])} traces, {sites['hit']} of {sites['total']} raise statements hit, "
          f"{os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    main()
