"""What time-varying edge weights cost on the streaming path (profiles/r22/tv_runs.txt).

    python tools/tv_time.py [--iters 6] [--reps 7] [--batch 512] [--out FILE]

Problem: the graph and the synthetic inputs of bench.py's cfg3 (N = 10 000, T = 24, t_in = 12, B = 512), float32, a fixed count
of ADMM iterations, ms per ADMM iteration.  Legs, one instance each in one process, alternated --reps times after one untimed
solve of every leg; a timed figure is one solve between two device synchronisations (host clock):
  a  time-invariant graph, the default plan (k_tile, the fused k_cldr, the folded vector updates);
  b  the same graph under MGADMM_TILE=0: plain row kernels (k_rows), two-pass Ldr^T Ldr, separate EpiPUpdate;
  c  the same weights as T / T-1 equal slices kept on the per-slice path (time_varying=True, MGADMM_TV_KEEP=1): the plan of b
     with k_rows_tv in place of k_rows on the same iterates (x equals b's bit for bit), so c - b is the cost of the slices;
  d  tables that really vary (slice t at sigma (1 + 0.05 t)): another problem with other CG counts, for information.
c is judged against b; a against c is the price of leaving the tiles and the fused kernel.
Prints one JSON line (and writes it to --out): the legs' figures, min / median / max, whether b and c agree bit for bit.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--reps", type=int, default=7, help="timed solves per leg")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    for p in (HERE, os.path.join(HERE, "mixed-graph-admm_amd")):
        sys.path.insert(0, p)
    import torch
    import bench
    import mgadmm
    from mgadmm import _lib as L
    dev = torch.device("cuda", 0)
    n, _, cl, dl, info, _ = bench.build_problem("cfg3")
    T, sigma = 24, 50.0
    y = bench.synth_y(n, args.batch, 12, 0, 0, dev)

    def instance(time_varying=False):
        blk = mgadmm.ADMM_algorithm({"n_nodes": n}, info, use_kNN=True, k=4, u_sigma=sigma, d_sigma=sigma, tables=(cl, dl), device=dev,
                                    compute_dtype=torch.float32, record_cg_coeffs=False, time_varying=time_varying)
        blk.check_stop, blk.max_ADMM_iter = False, args.iters
        return blk

    def solve(blk):
        blk._reset_history()
        return blk.combined_loop(y, print_info=False)

    # the switches are read when graph and solver are created, at an instance's first solve
    legs, first = {}, {}
    for name, tv, env in (("a", False, {}), ("b", False, {"MGADMM_TILE": "0"}), ("c", True, {"MGADMM_TV_KEEP": "1"}), ("d", True, {})):
        blk = instance(tv)
        if name == "d":
            per = [blk._weight_tables(sigma * (1 + 0.05 * t), sigma * (1 + 0.05 * t)) for t in range(T)]
            blk.u_ew = torch.stack([u[0] for u, _, _ in per])
            blk.d_ew = torch.stack([d[0] for _, d, _ in per[:T - 1]])
        os.environ.update(env)
        try:
            first[name] = solve(blk)
            torch.cuda.synchronize()
        finally:
            for k in env:
                del os.environ[k]
        legs[name] = blk
    h = {name: blk._solvers[(1, torch.float32)][0] for name, blk in legs.items()}
    plan = {name: dict(tile_rows=L.query(h[name], L.Q_TILE_ROWS), cldr_slots=L.query(h[name], L.Q_CLDR_SLOTS),
                       time_varying=bool(legs[name]._graphs[1][0].time_varying)) for name in legs}
    ms = {name: [] for name in legs}
    for _ in range(args.reps):
        for name, blk in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            solve(blk)
            torch.cuda.synchronize()
            ms[name].append(round((time.perf_counter() - t0) * 1e3 / args.iters, 3))
    cg = {name: int(torch.stack(blk.CG_iter_x).sum() + torch.stack(blk.CG_iter_zu).sum() + torch.stack(blk.CG_iter_zd).sum())
          for name, blk in legs.items()}
    res = dict(lib=L.version(), N=n, B=args.batch, T=T, iters=args.iters, reps=args.reps, plan=plan,
               b_equals_c=bool(torch.equal(first["b"], first["c"])), cg_iterations_summed=cg,
               ms_per_iteration=ms,
               summary={name: dict(min=min(v), median=round(statistics.median(v), 3), max=max(v)) for name, v in ms.items()})
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
