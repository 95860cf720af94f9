#!/usr/bin/env python3
"""Generate g11_time_varying.npz by IMPORTING AND RUNNING the reference on weight tables that vary over time.

Run where gen_golden.py runs (it imports the reference the same way, through gen_golden):

    cd /tmp && MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/gen_golden_tv.py

The reference's operators broadcast u_ew of shape (T, N, k) and d_ew of shape (T-1, N, k+1) slice by slice (ADMM.py:147, 171,
200, 214); its constructor only ever stores repeats of one slice.  Here the tables of an instance are REPLACED after
construction: slice t is the reference's own undirected_graph_from_distance / directed_graph_from_distance at
sigma * (1 + 0.05 t), so adjacent slices differ in every entry.  Graph: the one of g4_meta.npz (N = 30, k = 4, sigma = 50).
Modes knn and physical (the reference always has quirk Q1: bug_compat on).

  {mode}_cl, {mode}_u_ew (24, N, k), {mode}_d_ew (23, N, k+1)     the tables (T = 4 uses the first 4 / 3 slices)
  ops/{mode}/Lu, Ldr, Ldr_T, cLdr, LHS_x, LHS_x_mask, LHS_zu, LHS_zd    dense matrices at T = 4, t_in = 2; ops/mask
  cg/{mode}/{x,xmask,zu,zd}_{x,iters,alpha,beta}, cg/rhs, cg/x0    one CG_solver run per left-hand side at T = 4
  {mode}-None-{pred,mask}-f64-10/...                               combined_loop at T = 24, t_in = 12, 10 iterations: what
                                                                   gen_golden.run_solve stores for g4_solves.npz
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (imports the reference)

torch, ref_utils = gg.torch, gg.ref_utils
OUT = os.path.dirname(os.path.abspath(__file__))
GROWTH = 0.05


def vary(a, sigma, T):
    """Replace the tables of the reference instance `a` by T / T-1 slices at sigma * (1 + GROWTH t)."""
    cl, dl = a.connect_list, a.dist_list
    a.u_ew = torch.stack([gg.quiet(ref_utils.undirected_graph_from_distance, cl, dl, u_sigma=sigma * (1 + GROWTH * t)) for t in range(T)])
    a.d_ew = torch.stack([gg.quiet(ref_utils.directed_graph_from_distance, cl, dl, d_sigma=sigma * (1 + GROWTH * t)) for t in range(T - 1)])
    assert not bool((a.u_ew[1:] == a.u_ew[:-1])[a.u_ew[1:] != 0].any()) and not bool((a.d_ew[1:] == a.d_ew[:-1])[a.d_ew[1:] != 0].any())
    return a


def main():
    meta = np.load(os.path.join(OUT, "g4_meta.npz"))
    n, k, sigma = int(meta["n"]), int(meta["k"]), float(meta["sigma"])
    gi = gg.graph_info(n, meta["edges"], meta["dist"])
    full = torch.from_numpy(meta["x_true"])
    mask = torch.from_numpy(meta["mask"])
    out = {"n": n, "k": k, "sigma": sigma, "growth": GROWTH}
    T4, tin4 = 4, 2
    torch.manual_seed(7)
    m4 = (torch.rand(1, T4, n, 1, dtype=torch.float64) >= 0.4).float()
    out["ops/mask"] = m4.numpy()
    torch.manual_seed(11)
    rhs = torch.randn(1, T4, n, 1, dtype=torch.float64) * 10
    x0 = torch.randn(1, T4, n, 1, dtype=torch.float64)
    out["cg/rhs"], out["cg/x0"] = rhs.numpy(), x0.numpy()
    for mode in ("knn", "physical"):
        info4 = gg.admm_info(n, T4)
        a = vary(gg.build(gi, info4, mode, k, sigma, t_in=tin4, T=T4), sigma, T4)
        for nm in ("Lu", "Ldr", "Ldr_T", "cLdr"):
            out[f"ops/{mode}/{nm}"] = gg.dense_of(getattr(a, "apply_op_" + nm), T4, n)
        out[f"ops/{mode}/LHS_x"] = gg.dense_of(a.LHS_x, T4, n)
        out[f"ops/{mode}/LHS_x_mask"] = gg.dense_of(lambda e: a.LHS_x(e, mask=m4), T4, n)
        out[f"ops/{mode}/LHS_zu"] = gg.dense_of(a.LHS_zu, T4, n)
        out[f"ops/{mode}/LHS_zd"] = gg.dense_of(a.LHS_zd, T4, n)
        for nm, fn, kw in (("x", a.LHS_x, {}), ("xmask", a.LHS_x, {"mask": m4.double()}), ("zu", a.LHS_zu, {}), ("zd", a.LHS_zd, {})):
            x, it, al, be = a.CG_solver(fn, rhs, x0, **kw)
            out[f"cg/{mode}/{nm}_x"], out[f"cg/{mode}/{nm}_iters"] = x.numpy(), it
            out[f"cg/{mode}/{nm}_alpha"] = np.asarray([float(v) for v in al])
            out[f"cg/{mode}/{nm}_beta"] = np.asarray([float(v) for v in be])
        for key in ("rho", "rho_u", "rho_d", "mu_u", "mu_d1", "mu_d2"):
            out[f"ops/{key}"] = info4[key]
        T, t_in = int(meta["T"]), int(meta["t_in"])
        info = gg.admm_info(n, T)
        for task in ("pred", "mask"):
            a = vary(gg.build(gi, info, mode, k, sigma, t_in=t_in, T=T), sigma, T)
            if task == "pred":
                y, m = full[:, :t_in].double(), None
            else:
                y, m = (full * mask).double(), mask.clone()
            res = gg.run_solve(a, y, m, 10)
            for kk, v in res.items():
                out[f"{mode}-None-{task}-f64-10/{kk}"] = v
            print(mode, task, "CG", res["CG_iter_x"][-1], res["CG_iter_zu"][-1], "pri", res["p_res"][-1], file=sys.stderr)
        out[f"{mode}_cl"], out[f"{mode}_u_ew"], out[f"{mode}_d_ew"] = a.connect_list.numpy(), a.u_ew.numpy(), a.d_ew.numpy()
    out["T"], out["t_in"], out["T_ops"], out["t_in_ops"] = int(meta["T"]), int(meta["t_in"]), T4, tin4
    path = os.path.join(OUT, "g11_time_varying.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
