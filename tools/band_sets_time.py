"""What a sweep over the skip-connection interval costs as one batch with per-sample band tables, against one instance per
interval solved in a loop (the shape of profiles/r18/band_timing.json).

    python tools/band_sets_time.py [--windows 16] [--iters 50] [--reps 9] [--inner 10] [--out FILE]

Problem: the graph and the synthetic inputs of bench.py's cfg2 (N = 307, T = 24, t_in = 12) as a line graph, W windows, the
six intervals 1 .. 6, a fixed count of ADMM iterations, float32.

Legs, in one process, alternated --reps times; each timed figure is the mean of --inner solves, every solve between two
device synchronisations (host clock), after one untimed pass of every leg:
  batch  one solve of B = 6 W on the width-6 instance with band_params (kernels k_admm_lds_pp);
  loop   six solves of B = W, one per instance of the native width (k_admm_lds): the way without the feature;
  plain  the B = 6 W solve of the width-6 instance without a table (k_admm_lds): what the table costs.
Prints one JSON line (and writes it to --out): the legs' times in ms per sweep, their medians, whether batch and loop agree
bit for bit, and the unit and instance the batch ran.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTERVALS = (1, 2, 3, 4, 5, 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9, help="timed figures per leg")
    ap.add_argument("--inner", type=int, default=10, help="solves per timed figure")
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    for p in (HERE, os.path.join(HERE, "mixed-graph-admm_amd")):
        sys.path.insert(0, p)
    import torch
    import bench
    import mgadmm
    from mgadmm import _lib as L
    dev = torch.device("cuda", 0)
    n, _, cl, dl, info, _ = bench.build_problem("cfg2")
    W = args.windows

    def instance(skip):
        blk = mgadmm.ADMM_algorithm({"n_nodes": n}, info, use_kNN=True, k=4, u_sigma=50, d_sigma=50, tables=(cl, dl), device=dev,
                                    compute_dtype=torch.float32, record_cg_coeffs=False, use_line_graph=True, skip_connection=skip)
        blk.check_stop, blk.max_ADMM_iter = False, args.iters
        return blk

    wide = instance(INTERVALS[-1])
    native = [instance(s) for s in INTERVALS]
    yw = bench.synth_y(n, W, 12, 0, 0, dev)
    yall = yw.repeat(len(INTERVALS), 1, 1, 1)                     # sample b: interval b // W on window b % W
    skips = [s for s in INTERVALS for _ in range(W)]

    def solve(blk, y, **kw):
        blk._reset_history()
        return blk.combined_loop(y, print_info=False, **kw)

    legs = {"batch": lambda: solve(wide, yall, band_params={"skip": skips}),
            "loop": lambda: torch.cat([solve(blk, yw) for blk in native]),
            "plain": lambda: solve(wide, yall)}

    def timed(run, count):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            x = run()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / count, x

    x = {name: timed(legs[name], 1)[1] for name in ("plain", "loop", "batch")}     # the warm-up pass; the batch runs last ...
    h = wide._solvers[(1, torch.float32)][0]                                        # ... so these two report its launches
    unit, inst = L.query(h, L.Q_LDS_UNIT), L.lds_instance(h)
    ms = {name: [] for name in legs}
    for _ in range(args.reps):
        for name, run in legs.items():
            ms[name].append(round(timed(run, args.inner)[0], 3))
    res = dict(lib=L.version(), N=n, B=len(skips), windows=W, iters=args.iters, reps=args.reps, inner=args.inner,
               equal=bool(torch.equal(x["batch"], x["loop"])), unit_batch=unit, instance=inst,
               **{f"{name}_ms": v for name, v in ms.items()},
               **{f"{name}_median_ms": round(statistics.median(v), 3) for name, v in ms.items()})
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
