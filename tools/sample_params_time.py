"""What a hyperparameter sweep costs as one batch with per-sample ADMM weights, against one solve per parameter set.

    python tools/sample_params_time.py [--windows 16] [--sets 256] [--iters 50] [--inner 3]

Problem: the graph and the synthetic inputs of bench.py's cfg2 (N = 307, T = 24, t_in = 12), W windows, P parameter sets: a
square grid over mu_u x mu_d1, each from a quarter to four times the workload's value; a fixed count of ADMM iterations.

Legs, one fresh process each with a time limit of its own (--leg-timeout), one after the other; a leg that fails ends the run:
  loop   P solves of B = W in a Python loop, the scalars reassigned before every solve (the way without the feature);
  table  one solve of B = P * W with sample_params (k_admm_lds_pp);
  plain  the same B = P * W solve without a table (k_admm_lds): what the table loads cost.
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
    from mgadmm import _lib as L
    dev = torch.device("cuda", 0)
    n, _, cl, dl, info, _ = bench.build_problem("cfg2")
    W, P = args.windows, args.sets
    side = int(round(P ** 0.5))
    assert side * side == P, "--sets must be a square number"
    f = np.geomspace(0.25, 4.0, side)
    sets = [dict(mu_u=info["mu_u"] * a, mu_d1=info["mu_d1"] * b) for a, b in itertools.product(f, f)]
    blk = bench.make_solver(n, cl, dl, info, dev)
    blk.max_ADMM_iter = args.iters
    yw = bench.synth_y(n, W, 12, 0, 0, dev)
    yall = yw.repeat(P, 1, 1, 1)                                  # sample s = set s // W on window s % W
    table = {k: np.repeat([s[k] for s in sets], W) for k in ("mu_u", "mu_d1")}

    def one_pass():
        if args.leg == "loop":
            out = []
            for s in sets:
                blk.mu_u, blk.mu_d1 = s["mu_u"], s["mu_d1"]
                blk._reset_history()
                out.append(blk.combined_loop(yw, print_info=False))
            return torch.cat(out)
        blk._reset_history()
        return blk.combined_loop(yall, print_info=False, sample_params=table if args.leg == "table" else None)

    times = []
    for k in range(args.inner + 1):                               # the first pass is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = one_pass()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    h = blk._solvers[(1, torch.float32)][0]
    print(json.dumps(dict(leg=args.leg, lib=L.version(), W=W, P=P, B=W * P, iters=args.iters, instance=L.lds_instance(h),
                          ms=[round(t, 3) for t in times[1:]], warmup_ms=round(times[0], 3),
                          x_checksum=float(x.double().abs().mean()))), flush=True)


def child(name, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--windows", str(args.windows), "--sets", str(args.sets),
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
    ap.add_argument("--sets", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--inner", type=int, default=3, help="timed passes per process")
    ap.add_argument("--leg-timeout", type=float, default=240.0)
    ap.add_argument("--leg", choices=["loop", "table", "plain"])
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    res = {name: child(name, args) for name in ("loop", "table", "plain")}
    med = {k: statistics.median(v["ms"]) for k, v in res.items()}
    rng = {k: [min(v["ms"]), max(v["ms"])] for k, v in res.items()}
    # the loop's cells and the table's cells are the same solves: the checksums of x agree
    print(json.dumps(dict(summary=True, W=args.windows, P=args.sets, iters=args.iters, median_ms={k: round(v, 3) for k, v in med.items()},
                          range_ms=rng, loop_over_table=round(med["loop"] / med["table"], 2),
                          table_over_plain=round(med["table"] / med["plain"], 4),
                          same_x=res["loop"]["x_checksum"] == res["table"]["x_checksum"])), flush=True)


if __name__ == "__main__":
    main()
