"""Cases and the child-process worker of tests/test_gpu_lds_row_order.py (not a test module).

MGADMM_LDS_ROW_ORDER is read when a solver is planned, so every setting runs in a process of its own:
    python tests/lds_row_order_cases.py <case> <out.npz>
solves the case on the GPU and writes x, the exported state, the per-sample metric sums, the CG counts and the instance that ran.
The cases and `rows_moved` are also used without a GPU by tests/test_lds_rows_cpu.py, which holds `rows_moved` against the row
plan of csrc/lds_rows.h on the same graphs.
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

LISTS = ("CG_iter_x", "CG_iter_zu", "CG_iter_zd")
NLEAD = 5                              # LDS_NLEAD of csrc/lds_args.h
NODE, IN_DEGREE, TAIL_CLASS = 0, 1, 2  # ldsrows::Order = values of MGADMM_LDS_ROW_ORDER (unset: TAIL_CLASS)
CASES = ("cfg2", "cfg2mask", "hub0", "hub1", "hub2", "hub3", "aligned", "resume")


def rows_moved(cl, order):
    """How many LDS rows are another node than in node order under a row order (the stable sort of lds_rows.h, make_plan)."""
    import lds_census as lc
    deg = lc.in_degrees(np.asarray(cl))
    key = deg if order == IN_DEGREE else (np.maximum(deg - NLEAD, 0) + 1) // 2 if order == TAIL_CLASS else np.zeros_like(deg)
    node_of_row = np.argsort(-key, kind="stable")
    return int((node_of_row != np.arange(len(deg))).sum())


def _census_row(tp, slots=True):
    import lds_census as lc
    return next(r for r in lc.CENSUS if r["expect"] == lc.uni(8, 1024, slots, tp))


def case(name):
    """dict(N, T, t_in, B, abl, task, iters, tables, info, env, expect)"""
    import lds_census as lc
    if name == "cfg2":
        import bench
        n, _, cl, dl, info, _ = bench.build_problem("cfg2")
        return dict(N=n, T=24, t_in=12, B=96, abl="None", task="pred", iters=16, tables=(cl, dl), info=info,
                    env={"MGADMM_LDS_CHUNK": "16"}, expect=lc.uni(8, 1024, True, 2), sigma=50)
    if name == "cfg2mask":                          # the same graph (49 rows move under the default order): masked input, 'DGTV'
        import bench
        n, _, cl, dl, info, _ = bench.build_problem("cfg2")
        return dict(N=n, T=24, t_in=12, B=8, abl="DGTV", task="mask", iters=6, tables=(cl, dl), info=info, env={},
                    expect=lc.uni(8, 1024, True, 2), sigma=50)
    if name.startswith("hub"):                      # hub0 .. hub3: the census row of the TPG-8 slot instance with that tail
        r = _census_row(int(name[3:]))
        rr = math.sqrt(r["N"] / r["T"])
        info = dict(rho=2 * rr, rho_u=3 * rr, rho_d=2 * rr, mu_u=1, mu_d1=2, mu_d2=1)
        return dict(N=r["N"], T=r["T"], t_in=r["t_in"], B=5, abl=r["abl"], task=r["task"], iters=6, tables=lc.tables_for(r),
                    info=info, env=dict(r["env"]), expect=r["expect"], sigma=None)
    if name in ("aligned", "resume"):               # N = 128, G = 3: every time group starts a wave; in-degree 9 -> tail_pairs 2
        N, T = 128, 24
        rr = math.sqrt(N / T)
        info = dict(rho=2 * rr, rho_u=3 * rr, rho_d=2 * rr, mu_u=1, mu_d1=2, mu_d2=1)
        return dict(N=N, T=T, t_in=12, B=4, abl="None", task="mask" if name == "aligned" else "pred", iters=7,
                    tables=lc.uniform_tables(N, 9), info=info, env={}, expect=lc.uni(8, 1024, True, 2), sigma=None)
    raise SystemExit(f"unknown case {name}")


def inputs(c, seed=0):
    rng = np.random.default_rng(seed)
    x_true = (100 + 50 * rng.random((c["B"], c["T"], c["N"], 1))).astype(np.float32)
    if c["task"] == "pred":
        return x_true[:, :c["t_in"]].copy(), None
    mask = (rng.random(x_true.shape) >= 0.4).astype(np.float32)
    return x_true * mask, mask


def product(c):
    import mgadmm
    kw = dict(u_sigma=c["sigma"], d_sigma=c["sigma"]) if c["sigma"] else {}
    return mgadmm.ADMM_algorithm({"n_nodes": c["N"]}, c["info"], use_kNN=True, k=4, tables=c["tables"], ablation=c["abl"],
                                 t_in=c["t_in"], T=c["T"], record_cg_coeffs=False, path="lds", **kw)


# ------------------------------------------------------------------------------------------------ child process
def _worker(name, out_path):
    import torch
    from mgadmm import _lib
    c = case(name)
    for k, v in c["env"].items():
        os.environ[k] = v
    y, mask = inputs(c)
    yt = torch.from_numpy(y)
    mt = None if mask is None else torch.from_numpy(mask)
    blk = product(c)
    blk.check_stop = False

    def solve(iters, warm=None):
        blk.max_ADMM_iter = iters
        blk._reset_history()
        x = blk.solve(yt, mask=mt, per_sample_history=True, warm_start=warm)[0]
        return x.clone()

    out = {}
    x = solve(c["iters"])
    h = blk._solvers[(1, torch.float32)][0]
    assert _lib.lib.mgadmm_solver_path(h, c["B"]) == _lib.PATH_LDS
    out["instance"] = np.array(_lib.lds_instance(h))
    out["x"] = x.cpu().numpy()
    out["mps"] = np.asarray(blk.metrics_per_sample)
    for k in LISTS:
        vals = [np.asarray(v) for v in getattr(blk, k)]            # ('DGLR' runs no zd solve: an empty list)
        out[k] = np.stack(vals) if vals else np.zeros((0, c["B"]), dtype=np.int64)
    for k, v in blk.state.items():
        if v is not None:
            out["state_" + k] = v.cpu().numpy()
    if name == "resume":
        k1 = 4
        solve(k1)
        saved = {k: (None if v is None else v.clone()) for k, v in blk.state.items()}
        out["mps_first"] = np.asarray(blk.metrics_per_sample)
        x_res = solve(c["iters"] - k1, warm=saved)
        out["x_resumed"] = x_res.cpu().numpy()
        out["mps_second"] = np.asarray(blk.metrics_per_sample)
        for k, v in blk.state.items():
            if v is not None:
                out["resumed_state_" + k] = v.cpu().numpy()
    blk.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    _worker(sys.argv[1], sys.argv[2])


