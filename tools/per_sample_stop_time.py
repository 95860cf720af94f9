"""Time of a cfg2-shaped solve WITH the ADMM stop test: whole-batch stopping against per-sample stopping.

    python tools/per_sample_stop_time.py [--baseline-root DIR] [--repeats 5] [--batch 4096] [--target 50]

Problem: the graph and the synthetic inputs of bench.py's cfg2 (N = 307, T = 24, t_in = 12), sample b scaled by an amplitude
from a decade (10^u, u evenly spaced in [0, 1), shuffled with a fixed seed) so that the samples stop at different iterations;
ADMM_tol = the median over the samples of the largest per-sample residual after iteration `target` of a run without stop test
(the median sample stops near that iteration); max_ADMM_iter = 150.

Legs, one fresh process each, interleaved A B A B ... on one GPU: A = admm_convergence 'whole_batch' with check_stop (from
--baseline-root when given: another checkout of the project, e.g. the parent commit, with its own built library),
B = 'per_sample' from this tree.  Every process warms up with one untimed solve and times `--inner` solves (wall clock around
blk.combined_loop between device synchronisations).  Prints one JSON line per leg and a summary line: median / min / max of
the solve times, n_whole, sum of n_b and the iteration ratio B * n_whole / sum n_b.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def leg(args):
    root = os.path.abspath(args.root)
    for p in (root, os.path.join(root, "mixed-graph-admm_amd")):
        sys.path.insert(0, p)
    import time
    import numpy as np
    import torch
    import bench
    from mgadmm import _lib as L
    dev = torch.device("cuda", 0)
    n, _, cl, dl, info, _ = bench.build_problem("cfg2")
    B = args.batch
    blk = bench.make_solver(n, cl, dl, info, dev)
    u = torch.arange(B, dtype=torch.float32) / B
    amp = (10.0 ** u)[torch.randperm(B, generator=torch.Generator().manual_seed(7))]
    y = bench.synth_y(n, B, 12, 0, 0, dev) * amp.to(dev).reshape(B, 1, 1, 1)
    blk.max_ADMM_iter = 150
    out = dict(leg=args.leg, root=root, lib=L.version(), B=B)
    if args.leg == "calibrate":
        blk.check_stop, blk.max_ADMM_iter = False, args.target
        blk.solve(y, per_sample_history=True, return_state=False)
        row = blk.metrics_per_sample[args.target - 1]                     # (NMETRIC, B) sums of squares
        worst = np.sqrt(row[[L.M_PRI_ZU, L.M_DUAL_ZU, L.M_PRI_PHI, L.M_DUAL_PHI, L.M_PRI_ZD, L.M_DUAL_ZD]].max(0))
        out.update(tol=float(np.median(worst)), worst_min=float(worst.min()), worst_max=float(worst.max()))
        print(json.dumps(out), flush=True)
        return
    blk.check_stop, blk.ADMM_tol = True, args.tol
    if args.leg == "per_sample":
        blk.admm_convergence = "per_sample"
    times = []
    for k in range(args.inner + 1):                                         # the first solve is the warm-up
        blk._reset_history()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        blk.combined_loop(y, print_info=False)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    n_it = len(blk.p_res_list)
    nps = getattr(blk, "n_iters_per_sample", None)
    out.update(tol=args.tol, ms=[round(t, 3) for t in times[1:]], warmup_ms=round(times[0], 3), n_iters=n_it,
               sample_iterations=int(nps.astype(np.int64).sum()) if nps is not None else B * n_it)
    if nps is not None:
        out.update(n_b_min=int(nps.min()), n_b_median=float(np.median(nps)), n_b_max=int(nps.max()))
    print(json.dumps(out), flush=True)


def child(root, name, args, tol=0.0):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--root", root, "--batch", str(args.batch), "--target",
           str(args.target), "--inner", str(args.inner), "--tol", repr(tol)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"leg {name} ({root}) failed with status {r.returncode}")        # nothing more is started on the GPU
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-root", default=HERE, help="checkout that runs the whole_batch legs (default: this tree)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3, help="timed solves per process")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--target", type=int, default=50)
    ap.add_argument("--leg-timeout", type=float, default=240.0)
    ap.add_argument("--leg", choices=["calibrate", "whole_batch", "per_sample"])
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--tol", type=float, default=0.0)
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    tol = child(HERE, "calibrate", args)["tol"]
    A, Bl = [], []
    for _ in range(args.repeats):
        A.append(child(args.baseline_root, "whole_batch", args, tol))
        Bl.append(child(HERE, "per_sample", args, tol))
    ta = [t for r in A for t in r["ms"]]
    tb = [t for r in Bl for t in r["ms"]]
    st = lambda v: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), n=len(v))
    n_whole, sum_nb = A[-1]["n_iters"], Bl[-1]["sample_iterations"]
    print(json.dumps(dict(summary=True, B=args.batch, tol=tol, whole_batch_ms=st(ta), per_sample_ms=st(tb), n_whole=n_whole,
                          B_times_n_whole=args.batch * n_whole, sum_n_b=sum_nb,
                          iteration_ratio=round(args.batch * n_whole / sum_nb, 3),
                          time_ratio=round(statistics.median(ta) / statistics.median(tb), 3))), flush=True)


if __name__ == "__main__":
    main()
