#!/usr/bin/env python3
"""The reference's notebook / experiment flow (example-PEMS04.ipynb, experiment_0319.py) on the MI355X path:

    files -> TrafficDataset (series resident on the GPU) -> kNN graph -> ADMM_algorithm
          -> prediction of the next 12 steps for a whole batch of sliding windows
          -> grid search over two ADMM weights on the first 16 windows, all cells in one batch
          -> comparison of three rho ramps (weights that change per ADMM iteration) x mu_d1, again one batch
          -> interpolation of 40 % masked entries

The PEMS files are not redistributable, so the script writes a synthetic PEMS-shaped data set (distance csv,
sensor-id file, (T, N, 3) series) into a temporary directory first; point --data-folder at a real
PEMS0X folder (PEMS04.npz / PEMS04.csv) to run on the real thing.

    python examples/pems_workflow.py [--nodes 307 --steps 2000 --batch 256 --iters 50]
"""
import argparse
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mixed-graph-admm_amd"))

from mgadmm.ADMM import ADMM_algorithm            # noqa: E402   (was: from ADMM import *)
from mgadmm.dataset import TrafficDataset          # noqa: E402   (was: from utils import *)
from mgadmm.gpu_graph import k_nearest_neighbors   # noqa: E402


def write_synthetic_pems(folder, n, steps, seed=0):
    import pandas as pd
    rng = np.random.default_rng(seed)
    ids = 1000 + 3 * np.arange(n)
    e = [(i, i + 1) for i in range(n - 1)]
    have = set(e)
    while len(e) < n - 1 + n // 9:
        a, b = int(rng.integers(n)), int(rng.integers(n))
        if a != b and (a, b) not in have and (b, a) not in have:
            e.append((a, b)); have.add((a, b))
    e = np.array(e)
    pd.DataFrame({"from": ids[e[:, 0]], "to": ids[e[:, 1]], "cost": rng.uniform(3.0, 2900.0, len(e))}).to_csv(
        os.path.join(folder, "PEMS.csv"), index=False)
    np.savetxt(os.path.join(folder, "PEMS.txt"), ids, fmt="%d")
    t = np.arange(steps)[:, None]
    # neighbouring sensors see similar, slightly delayed traffic: level and phase vary smoothly along the path
    base = np.clip(220 + np.cumsum(rng.normal(0, 6, n)), 60, 400)[None, :]
    phase = np.cumsum(rng.normal(0, 0.15, n))[None, :]
    flow = base * (1 + 0.35 * np.sin(2 * np.pi * t / 288 + phase)) + 8 * rng.standard_normal((steps, n))
    data = np.stack([flow, rng.random((steps, n)), rng.random((steps, n))], -1)
    np.savez(os.path.join(folder, "PEMS.npz"), data=data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data-folder", default=None)
    ap.add_argument("--nodes", type=int, default=307)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--transform", default="none", choices=["none", "standardize", "normalize"],
                    help="TrafficDataset transform; the notebooks' ADMM weights are tuned for the raw scale")
    args = ap.parse_args()
    tmp = None
    if args.data_folder is None:
        tmp = tempfile.TemporaryDirectory()
        write_synthetic_pems(tmp.name, args.nodes, args.steps)
        folder, data_file, graph_csv, id_file = tmp.name, "PEMS.npz", "PEMS.csv", "PEMS.txt"
    else:
        name = os.path.basename(os.path.normpath(args.data_folder))
        folder, data_file, graph_csv, id_file = args.data_folder, name + ".npz", name + ".csv", None

    ds = TrafficDataset(folder, data_file, graph_csv, id_file=id_file, transform=None if args.transform == "none" else args.transform)
    n = ds.graph_info["n_nodes"]
    print(f"data shape: {tuple(ds.data.shape)} on {ds.data.device}, node number: {n}, edge number: {ds.graph_info['n_edges']}")
    nn, nd = k_nearest_neighbors(n, ds.graph_info["u_edges"], ds.graph_info["u_dist"], 4)
    print(f"nearest nodes: {tuple(nn.shape)}, nearest_dists: {tuple(nd.shape)}")

    r = math.sqrt(n / 24)
    admm_info = {"rho": 2 * r, "rho_u": 3 * r, "rho_d": 2 * r, "mu_u": 1, "mu_d1": 2, "mu_d2": 1}
    blk = ADMM_algorithm(ds.graph_info, admm_info, use_kNN=True, k=4, u_sigma=50, d_sigma=50)
    blk.max_ADMM_iter = args.iters

    starts = torch.arange(0, args.batch) * ((ds.data.shape[0] - 24) // args.batch)
    x_true, y = ds.get_predict_batch(starts)                      # (B, 24, N, 1), (B, 12, N, 1) on the GPU
    torch.cuda.synchronize(); t0 = time.perf_counter()
    x_hat = blk.combined_loop(y, print_info=False)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    its = len(blk.p_res_list)
    err = (ds.recover_data(x_hat[:, 12:]) - ds.recover_data(x_true[:, 12:])).abs()
    print(f"prediction: {args.batch} windows x {its} ADMM iterations in {dt * 1e3:.1f} ms ({args.batch * its / dt:,.0f} sample-iterations/s); "
          f"MAE of the 12 predicted steps {err.mean().item():.2f}, fit of the 12 observed steps ||Hx - y|| = {blk.recover_list[-1]:.3g}")
    print(f"  CG iterations x/zu/zd of the last ADMM iteration: {blk.CG_iter_x[-1].float().mean():.1f} / "
          f"{blk.CG_iter_zu[-1].float().mean():.1f} / {blk.CG_iter_zd[-1].float().mean():.1f}; "
          f"primal residuals {['%.3g' % v for v in blk.p_res_list[-1]]}")

    # the notebooks' grid search (one combined_loop per value there): 3 x 3 sets of (mu_u, mu_d1) on the first 16 windows as ONE
    # batch of 144 samples, every sample with its own weights
    nw = min(16, args.batch)
    grid_mu_d1 = [0.5 * admm_info["mu_d1"], admm_info["mu_d1"], 2 * admm_info["mu_d1"]]
    grid = {"mu_u": [0.5 * admm_info["mu_u"], admm_info["mu_u"], 2 * admm_info["mu_u"]], "mu_d1": grid_mu_d1}
    blk._reset_history()
    blk.admm_convergence = "per_sample"                           # the stop test of a sweep: every cell on its own residuals
    torch.cuda.synchronize(); t0 = time.perf_counter()
    xs, n_it, sets = blk.sweep(y[:nw], grid)                      # (9, nw, 24, N, 1), (9, nw), 9 dicts
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    blk.admm_convergence = "whole_batch"
    truth = ds.recover_data(x_true[:nw, 12:])
    mae = [(ds.recover_data(xs[p][:, 12:]) - truth).abs().mean().item() for p in range(len(sets))]
    print(f"sweep: {len(sets)} sets x {nw} windows x {int(n_it.max())} ADMM iterations in {dt * 1e3:.1f} ms; MAE of the 12 predicted steps")
    print("  mu_u \\ mu_d1 " + "".join(f"{v:>9.3g}" for v in grid["mu_d1"]))
    for i, a in enumerate(grid["mu_u"]):
        print(f"  {a:>13.3g} " + "".join(f"{mae[i * 3 + j]:>9.3f}" for j in range(3)))

    # the other knob of the notebooks is the graph itself: 3 values of u_sigma x 3 of mu_u, again ONE batch -- every distinct
    # sigma gets its own weight tables on the instance's neighbour lists, every sample reads the tables of its cell
    grid = {"u_sigma": [25.0, 50.0, 100.0], "mu_u": [0.5 * admm_info["mu_u"], admm_info["mu_u"], 2 * admm_info["mu_u"]]}
    blk._reset_history()
    blk.admm_convergence = "per_sample"
    torch.cuda.synchronize(); t0 = time.perf_counter()
    xs, n_it, sets = blk.sweep(y[:nw], grid)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    blk.admm_convergence = "whole_batch"
    mae = [(ds.recover_data(xs[p][:, 12:]) - truth).abs().mean().item() for p in range(len(sets))]
    print(f"sigma sweep: {len(sets)} cells x {nw} windows x {int(n_it.max())} ADMM iterations in {dt * 1e3:.1f} ms; MAE of the 12 predicted steps")
    print("  u_sigma \\ mu_u " + "".join(f"{v:>9.3g}" for v in grid["mu_u"]))
    for i, a in enumerate(grid["u_sigma"]):
        print(f"  {a:>14.3g} " + "".join(f"{mae[i * 3 + j]:>9.3f}" for j in range(3)))

    # a varying penalty, the first thing anyone tunes in ADMM: rho, rho_u and rho_d ramped TOGETHER by a factor per iteration
    # (held after 30 rows), 3 factors x 3 values of mu_d1 on the same windows, again ONE batch with per-sample stopping --
    # column s of the (30, B) schedule is the ramp of sample s's cell; without the schedule every candidate is its own chain of
    # one-iteration solves
    from mgadmm.ADMM import geometric_ramp
    factors, mus = [1.0, 1.05, 1.1], grid_mu_d1
    cells = [(f, m) for f in factors for m in mus]                # cell p on window w: sample p * nw + w
    sched = {nm: np.stack([geometric_ramp(admm_info[nm], f, 30) for f, _ in cells for _ in range(nw)], axis=1)
             for nm in ("rho", "rho_u", "rho_d")}
    blk._reset_history()
    blk.admm_convergence = "per_sample"
    torch.cuda.synchronize(); t0 = time.perf_counter()
    blk.solve(y[:nw].repeat(len(cells), 1, 1, 1), return_state=False, param_schedule=sched,
              sample_params={"mu_d1": [m for _, m in cells for _ in range(nw)]})
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    blk.admm_convergence = "whole_batch"
    n_it = np.asarray(blk.n_iters_per_sample).reshape(len(cells), nw)
    print(f"rho ramps: {len(cells)} cells x {nw} windows in {dt * 1e3:.1f} ms; mean ADMM iterations to the tolerance {blk.ADMM_tol:g} per cell")
    print("  factor \\ mu_d1 " + "".join(f"{v:>9.3g}" for v in mus))
    for i, f in enumerate(factors):
        print(f"  {f:>14.3g} " + "".join(f"{n_it[i * 3 + j].mean():>9.1f}" for j in range(3)))

    # the solver chooses the penalties itself: residual balancing per sample on the device, a step after every 4th iteration
    # (between two kernel launches; no host round trip).  rho_history: (periods, 3, B) = rho, rho_u, rho_d by period
    blk._reset_history()
    blk.admm_convergence = "per_sample"
    torch.cuda.synchronize(); t0 = time.perf_counter()
    blk.solve(y[:nw], return_state=False, adaptive_rho={"every": 4, "mu": 10, "tau": 2})
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    blk.admm_convergence = "whole_batch"
    print(f"adaptive penalties: {nw} windows in {dt * 1e3:.1f} ms, {np.asarray(blk.n_iters_per_sample).mean():.1f} ADMM iterations on average; "
          f"rho, rho_u, rho_d of window 0 at the end: " + ", ".join(f"{v:.3g}" for v in blk.rho_final[:, 0])
          + f" (start: {admm_info['rho']:.3g}, {admm_info['rho_u']:.3g}, {admm_info['rho_d']:.3g})")

    # the grid search the reference's authors call their main finding is over the temporal graph itself: the largest
    # skip-connection interval of the line graph, 1 ... 6 (one instance, one graph and one solve per value there).  Here ONE
    # line-graph instance of width 6 and ONE batch: 6 intervals x 2 values of mu_d1 on the same windows, every sample reading the
    # band table of its interval (a narrower interval is the width-6 table with zero hops)
    line = ADMM_algorithm(ds.graph_info, admm_info, use_kNN=True, k=4, u_sigma=50, use_line_graph=True, skip_connection=6)
    line.max_ADMM_iter, line.admm_convergence = args.iters, "per_sample"
    skips, mus = [1, 2, 3, 4, 5, 6], [admm_info["mu_d1"], 2 * admm_info["mu_d1"]]
    torch.cuda.synchronize(); t0 = time.perf_counter()
    xs, n_it, sets = line.sweep(y[:nw], {"mu_d1": mus}, skips=skips)      # (12, nw, 24, N, 1); sets: mu_d1 slowest, 'skip' fastest
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    mae = [(ds.recover_data(xs[p][:, 12:]) - truth).abs().mean().item() for p in range(len(sets))]
    print(f"skip-connection sweep: {len(sets)} cells x {nw} windows x {int(n_it.max())} ADMM iterations in {dt * 1e3:.1f} ms; "
          "MAE of the 12 predicted steps / mean ADMM iterations")
    print("  mu_d1 \\ skip " + "".join(f"{s:>14d}" for s in skips))
    for i, m in enumerate(mus):
        print(f"  {m:>12.3g} " + "".join(f"{mae[i * 6 + j]:>8.3f} /{n_it[i * 6 + j].mean():>4.0f}" for j in range(6)))
    line.close()

    ix, iy, mask = ds.get_interpolated_batch(starts, 0.4)
    blk._reset_history()
    x_int = blk.combined_loop(iy, mask=mask, print_info=False)
    hidden = mask == 0
    e_int = (ds.recover_data(x_int) - ds.recover_data(ix)).abs()[hidden]
    print(f"interpolation (40 % masked): MAE on the hidden entries {e_int.mean().item():.2f}, "
          f"GLR / DGTV / DGLR = {blk.GLR_list[-1].item():.4g} / {blk.DGTV_list[-1].item():.4g} / {blk.DGLR_list[-1].item():.4g}")
    blk.close()
    if tmp is not None:
        tmp.cleanup()
    return err.mean().item(), e_int.mean().item()


if __name__ == "__main__":
    main()
