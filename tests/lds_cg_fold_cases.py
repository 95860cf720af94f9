"""Cases and the child-process worker of tests/test_gpu_lds_cg_fold.py (not a test module).

The uniform-row instances of k_admm_lds form p . A p of the cLdr solves from q . q ahead of the q exchange (three barriers per
CG iteration, MGADMM_Q_LDS_CG_BARRIERS); MGADMM_LDS_RAGGED=1 plans the generic instance of the same library for the same
graph (four barriers, p . A p after the W_d^T gather).  The switch is read when a solver is planned, so every leg runs in a
process of its own:
    python tests/lds_cg_fold_cases.py <case> <out.npz>
solves the case on the GPU and writes x, the exported state, the per-sample metric sums, the CG counts, the instance that ran
and what the plan queries say.  The graph cases are those of lds_row_order_cases.py plus the three ablations and a TPG 12 case
on its N = 128 graph; 'pp' / 'ps' / 'physical' run on the golden tables of g4_meta.npz (N = 30, k = 4 without pads).
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "mixed-graph-admm_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import lds_row_order_cases as rc          # noqa: E402
from lds_row_order_cases import LISTS     # noqa: E402

GRAPH_CASES = ("cfg2", "cfg2mask", "aligned", "hub0", "hub1", "hub2", "hub3", "DGTV", "DGLR", "UT", "tpg12")
PP_ITERS = 12
PS_TOL, PS_MAX_IT, PS_SINGLES = 7.348, 150, (0, 3, 6)      # test_gpu_admm_per_sample.py, TABLE[0]: ('knn', 'None')
# rows of the sample_params table, as factors of the fixture's weights (rho, rho_u, rho_d, mu_u, mu_d1, mu_d2)
PP_NAMES = ("rho", "rho_u", "rho_d", "mu_u", "mu_d1", "mu_d2")
PP_ROWS = np.array([[1.0, 1.0, 1.0, 1.0, 1.0, 1.0], [2.0, 1.0, 1.0, 1.0, 1.0, 1.0], [0.5, 1.0, 1.0, 1.0, 1.0, 1.0],
                    [1.0, 2.0, 0.5, 1.0, 1.0, 1.0], [1.0, 0.5, 2.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 2.0, 0.5, 1.0],
                    [1.0, 1.0, 1.0, 0.5, 2.0, 2.0], [1.5, 0.75, 1.25, 0.25, 4.0, 0.5]])


def case(name):
    """The dict of lds_row_order_cases.case, plus `ragged`: the instance MGADMM_LDS_RAGGED=1 runs."""
    import lds_census as lc
    if name in ("DGTV", "DGLR", "UT", "tpg12"):       # the N = 128 graph of 'aligned' (in-degree 9: tail_pairs 2)
        N, T = 128, 24
        rr = math.sqrt(N / T)
        info = dict(rho=2 * rr, rho_u=3 * rr, rho_d=2 * rr, mu_u=1, mu_d1=2, mu_d2=1)
        t12 = name == "tpg12"
        c = dict(N=N, T=T, t_in=12, B=4, abl="None" if t12 else name, task="mask" if name == "DGLR" else "pred", iters=7,
                 tables=lc.uniform_tables(N, 9), info=info, env={"MGADMM_LDS_TPG": "12"} if t12 else {}, sigma=None,
                 expect=lc.uni(12, 640, True, 2) if t12 else lc.uni(8, 1024, True, 2))
    else:
        c = rc.case(name)
    tpg, maxt = (12, 640) if name == "tpg12" else (8, 1024)
    c["ragged"] = lc.inst(tpg, False, maxt, False)
    return c


def g4_meta(physical_on_knn_tables=False):
    m = dict(np.load(os.path.join(HERE, "golden", "g4_meta.npz"), allow_pickle=False))
    if physical_on_knn_tables:        # use_kNN=False on the k = 4 table without pads: the rows qualify for a uniform instance
        assert (m["knn_cl"] != -1).all() and m["knn_cl"].shape[1] == 5
        m["phys_cl"], m["phys_u_ew"], m["phys_d_ew"] = m["knn_cl"], m["knn_u_ew"], m["knn_d_ew"]
    return m


def g5_y():
    return np.load(os.path.join(HERE, "golden", "g5_batched.npz"), allow_pickle=False)["y"].astype(np.float32)


def pp_table(meta):
    return {nm: np.array([float(meta[nm]) * r[j] for r in PP_ROWS]) for j, nm in enumerate(PP_NAMES)}


# ------------------------------------------------------------------------------------------------ child process
def _plan(out, blk, B):
    import torch
    from mgadmm import _lib
    h = blk._solvers[(1, torch.float32)][0]
    assert _lib.lib.mgadmm_solver_path(h, B) == _lib.PATH_LDS
    out["instance"] = np.array(_lib.lds_instance(h))
    out["barriers"] = np.array(_lib.query(h, _lib.Q_LDS_CG_BARRIERS))
    out["uniform"] = np.array(_lib.query(h, _lib.Q_LDS_UNIFORM))


def _collect(out, blk, x, prefix=""):
    out[prefix + "x"] = x.cpu().numpy()
    out[prefix + "mps"] = np.asarray(blk.metrics_per_sample)
    for k in LISTS:
        vals = [np.asarray(v).reshape(-1) for v in getattr(blk, k)]            # ('DGLR' runs no zd solve: an empty list)
        out[prefix + k] = np.stack(vals) if vals else np.zeros((0, x.shape[0]), dtype=np.int64)
    for k, v in blk.state.items():
        if v is not None:
            out[prefix + "state_" + k] = v.cpu().numpy()


def _graph_case(name, out):
    import torch
    c = case(name)
    for k, v in c["env"].items():
        os.environ[k] = v
    y, mask = rc.inputs(c)
    blk = rc.product(c)
    blk.check_stop = False
    blk.max_ADMM_iter = c["iters"]
    blk._reset_history()
    x = blk.solve(torch.from_numpy(y), mask=None if mask is None else torch.from_numpy(mask), per_sample_history=True)[0]
    _plan(out, blk, c["B"])
    _collect(out, blk, x)
    blk.close()


def _g4_case(name, out):
    import torch
    from helpers import make_product
    y = torch.from_numpy(g5_y())
    meta = g4_meta(physical_on_knn_tables=name == "physical")
    kw = dict(admm_convergence="per_sample") if name == "ps" else {}
    blk = make_product(meta, "physical" if name == "physical" else "knn", path="lds", **kw)
    blk.record_cg_coeffs = False              # the chunked schedule (several iterations per launch)
    if name == "ps":
        blk.max_ADMM_iter, blk.ADMM_tol = PS_MAX_IT, PS_TOL
    else:
        blk.max_ADMM_iter, blk.check_stop = PP_ITERS, False
    blk._reset_history()
    x = blk.solve(y, per_sample_history=True, sample_params=pp_table(meta) if name == "pp" else None)[0]
    _plan(out, blk, y.shape[0])
    _collect(out, blk, x)
    if name == "ps":
        out["n"] = blk.n_iters_per_sample.copy()
        blk.admm_convergence = "whole_batch"
        for b in PS_SINGLES:              # the same samples solved alone
            blk._reset_history()
            x1 = blk.solve(y[b:b + 1], per_sample_history=True)[0]
            out[f"single{b}_n"] = np.array(len(blk.p_res_list))
            _collect(out, blk, x1, prefix=f"single{b}_")
    blk.close()


if __name__ == "__main__":
    res = {}
    (_graph_case if sys.argv[1] in GRAPH_CASES else _g4_case)(sys.argv[1], res)
    np.savez(sys.argv[2], **res)
