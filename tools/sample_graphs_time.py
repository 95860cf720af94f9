"""What a sweep over the graph's sigmas costs as one batch with per-sample graph weights, against one instance per sigma pair
(DESIGN.md 3e).

    python tools/sample_graphs_time.py [--windows 16] [--side 16] [--iters 50] [--inner 3]

Problem: the tables and the synthetic inputs of bench.py's cfg2 (N = 307, T = 24, t_in = 12), W windows, side x side pairs
(u_sigma, d_sigma), each sigma from a quarter to four times the workload's 50; a fixed count of ADMM iterations.

Legs, one fresh process each with a time limit of its own (--leg-timeout), one after the other; a leg that fails ends the run:
  loop   one instance per pair, constructed and solved at B = W in a Python loop (the way without the feature); the time of
         constructing the instance and its solver (tables, device graph, planner run) and the time of the solves are reported
         separately;
  table  one solve of B = side^2 * W with graph_params (k_admm_lds_pp, one image per pair); the time includes building the
         tables and planning every pair, which a solve does anew;
  plain  the same batch on one graph without a table (k_admm_lds): what side^2 distinct images cost against one shared image.
Every process warms up untimed (one pass of its leg) and times --inner passes (wall clock between device synchronisations).
Prints one JSON line per leg and a summary line with the medians and the ratios loop / table and table / plain.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def leg(args):
    for p in (HERE, os.path.join(HERE, "mixed-graph-admm_amd")):
        sys.path.insert(0, p)
    import itertools
    import time
    import numpy as np
    import torch
    import bench
    import mgadmm
    from mgadmm import _lib as L
    dev = torch.device("cuda", 0)
    n, _, cl, dl, info, _ = bench.build_problem("cfg2")
    W, side = args.windows, args.side
    f = np.geomspace(0.25, 4.0, side)
    pairs = [(50.0 * a, 50.0 * b) for a, b in itertools.product(f, f)]
    P = len(pairs)
    yw = bench.synth_y(n, W, 12, 0, 0, dev)
    yall = yw.repeat(P, 1, 1, 1)                                  # sample s = pair s // W on window s % W
    gp = {"u_sigma": np.repeat([p[0] for p in pairs], W), "d_sigma": np.repeat([p[1] for p in pairs], W)}
    blk = bench.make_solver(n, cl, dl, info, dev)
    blk.max_ADMM_iter = args.iters
    split = {"build_ms": [], "solve_ms": []}

    def one_pass():
        if args.leg == "loop":
            out, tb, ts = [], 0.0, 0.0
            for us, ds in pairs:
                t0 = time.perf_counter()
                one = mgadmm.ADMM_algorithm({"n_nodes": n}, info, use_kNN=True, k=4, u_sigma=us, d_sigma=ds, tables=(cl, dl), device=dev,
                                            compute_dtype=torch.float32, record_cg_coeffs=False)
                one.check_stop, one.max_ADMM_iter = False, args.iters
                one._solver(1, torch.float32, W)
                t1 = time.perf_counter()
                out.append(one.combined_loop(yw, print_info=False))
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                one.close()
                tb += t1 - t0 + time.perf_counter() - t2
                ts += t2 - t1
            split["build_ms"].append(round(tb * 1e3, 3))
            split["solve_ms"].append(round(ts * 1e3, 3))
            return torch.cat(out)
        blk._reset_history()
        return blk.combined_loop(yall, print_info=False, **(dict(graph_params=gp) if args.leg == "table" else {}))

    times = []
    for k in range(args.inner + 1):                               # the first pass is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = one_pass()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    h = blk._solvers[(1, torch.float32)][0] if blk._solvers else None
    print(json.dumps(dict(leg=args.leg, lib=L.version(), W=W, P=P, B=W * P, iters=args.iters,
                          unit=None if h is None else L.query(h, L.Q_LDS_UNIT), ms=[round(t, 3) for t in times[1:]],
                          warmup_ms=round(times[0], 3), **{k: v[1:] for k, v in split.items() if v},
                          x_checksum=float(x.double().abs().mean()))), flush=True)


def child(name, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--windows", str(args.windows), "--side", str(args.side),
           "--iters", str(args.iters), "--inner", str(args.inner)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"leg {name} failed with status {r.returncode}")        # nothing more is started on the GPU
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--side", type=int, default=16, help="values per sigma: side^2 pairs")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--inner", type=int, default=3, help="timed passes per process")
    ap.add_argument("--leg-timeout", type=float, default=400.0)
    ap.add_argument("--leg", choices=["loop", "table", "plain"])
    ap.add_argument("--legs", default="loop,table,plain")
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    res = {name: child(name, args) for name in args.legs.split(",")}
    med = {k: statistics.median(v["ms"]) for k, v in res.items()}
    out = dict(summary=True, W=args.windows, P=args.side ** 2, iters=args.iters, median_ms={k: round(v, 3) for k, v in med.items()},
               range_ms={k: [min(v["ms"]), max(v["ms"])] for k, v in res.items()})
    if "loop" in res:
        out["loop_build_ms"] = statistics.median(res["loop"]["build_ms"])
        out["loop_solve_ms"] = statistics.median(res["loop"]["solve_ms"])
    if "loop" in res and "table" in res:
        out["loop_over_table"] = round(med["loop"] / med["table"], 2)
        out["same_x"] = res["loop"]["x_checksum"] == res["table"]["x_checksum"]      # the same solves: the checksums of x agree
    if "table" in res and "plain" in res:
        out["table_over_plain"] = round(med["table"] / med["plain"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
