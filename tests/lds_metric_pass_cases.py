"""Cases and the child-process worker of tests/test_gpu_lds_metric_pass.py (not a test module).

MGADMM_LDS_ASYNC and MGADMM_LDS_CHUNK are read when a solver is created, so every leg runs in a process of its own:
    python tests/lds_metric_pass_cases.py <case> <out.npz>
solves the case on the GPU under the environment it was started with and writes x, the exported state, every history list,
delta_x_per_step, the per-sample metric sums, the CG counts and the instance that ran.
Cases: `g4:<B>` -- the g4 kNN table (N = 30, T = 24: the uniform TPG-8 instance), prediction, 7 iterations, B windows made
from the golden ones; `rc:<name>` -- a case of lds_row_order_cases.py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "mixed-graph-admm_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

LISTS = ("p_res_list", "d_res_list", "x_shift_list", "GLR_list", "DGTV_list", "DGLR_list", "recover_list")
CG_LISTS = ("CG_iter_x", "CG_iter_zu", "CG_iter_zd")
G4_ITERS = 7


def g4_meta():
    return np.load(os.path.join(HERE, "golden", "g4_meta.npz"), allow_pickle=False)


def g4_inputs(meta, B):
    """B prediction windows: the golden ones, repeated with another amplitude and a little noise."""
    y = meta["x_true"][:, :int(meta["t_in"])].astype(np.float32)
    rng = np.random.default_rng(5)
    reps = -(-B // y.shape[0])
    y = np.concatenate([y * np.float32(1 + 0.01 * r) for r in range(reps)])[:B]
    return (y + (rng.random(y.shape) * 0.5).astype(np.float32)).astype(np.float32)


def g4_product(meta):
    """helpers.make_product(meta, 'knn', path='lds') without conftest (a child process must not start a build)."""
    import torch
    from mgadmm.ADMM import ADMM_algorithm
    info = {k: float(meta[k]) for k in ("rho", "rho_u", "rho_d", "mu_u", "mu_d1", "mu_d2")}
    T, t_in, n = int(meta["T"]), int(meta["t_in"]), int(meta["n"])
    cl = torch.from_numpy(meta["knn_cl"])
    blk = ADMM_algorithm({"n_nodes": n}, info, use_kNN=True, k=cl.shape[1] - 1, u_sigma=1.0, d_sigma=1.0, ablation="None", t_in=t_in,
                         T=T, tables=(cl, torch.zeros(cl.shape) + 1.0), compute_dtype=torch.float32, record_cg_coeffs=False, path="lds")
    blk.u_ew = torch.from_numpy(np.asarray(meta["knn_u_ew"], dtype=np.float32)).unsqueeze(0).repeat(T, 1, 1)
    blk.d_ew = torch.from_numpy(np.asarray(meta["knn_d_ew"], dtype=np.float32)).unsqueeze(0).repeat(T - 1, 1, 1)
    return blk


def problem(case):
    """(product, y, mask, iterations, B)"""
    kind, arg = case.split(":")
    if kind == "g4":
        meta = g4_meta()
        B = int(arg)
        return g4_product(meta), g4_inputs(meta, B), None, G4_ITERS, B
    import lds_row_order_cases as rc
    c = rc.case(arg)
    y, mask = rc.inputs(c)
    return rc.product(c), y, mask, c["iters"], c["B"]


def _worker(case, out_path):
    import torch
    from mgadmm import _lib
    blk, y, mask, iters, B = problem(case)
    blk.check_stop = False
    blk.max_ADMM_iter = iters
    x = blk.solve(torch.from_numpy(y), mask=None if mask is None else torch.from_numpy(mask), per_sample_history=True)[0]
    h = blk._solvers[(1, torch.float32)][0]
    assert _lib.lib.mgadmm_solver_path(h, B) == _lib.PATH_LDS
    out = {"instance": np.array(_lib.lds_instance(h)), "x": x.cpu().numpy(), "mps": np.asarray(blk.metrics_per_sample),
           "dxps": np.array([np.asarray(v) for v in blk.delta_x_per_step], dtype=np.float64)}
    for k in LISTS:
        out[k] = np.array([np.asarray(v) for v in getattr(blk, k)], dtype=np.float64)
    for k in CG_LISTS:
        vals = [np.asarray(v) for v in getattr(blk, k)]            # ('DGLR' runs no zd solve: an empty list)
        out[k] = np.stack(vals).reshape(len(vals), B) if vals else np.zeros((0, B), dtype=np.int64)
    for k, v in blk.state.items():
        if v is not None:
            out["state_" + k] = v.cpu().numpy()
    blk.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    _worker(sys.argv[1], sys.argv[2])
