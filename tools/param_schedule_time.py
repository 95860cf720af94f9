"""What a rho ramp costs as one scheduled solve, against the chain of one-iteration solves it replaces and against the same
solve without a schedule.

    python tools/param_schedule_time.py [--batch 4096] [--iters 50] [--inner 3] [--factor 1.03]

Problem: the tables and the synthetic inputs of bench.py's cfg2 (N = 307, T = 24, t_in = 12), B samples, a fixed count of
ADMM iterations; rho, rho_u and rho_d ramped together by --factor (1.03) per row over `iters` rows (shared form).  A ramp
changes the CG iteration counts, so `schedule` and `plain` then do different work; --factor 1 makes every row the scalars:
the same arithmetic in both legs, the ratio is what reading the weights by row costs.

Legs, one fresh process each with a time limit of its own (--leg-timeout), one after the other; a leg that fails ends the run:
  chain      `iters` solves of one iteration, resumed with warm_start=, the row's three rhos assigned as scalars between them
             (the way without the feature: k_admm_lds, one iteration per launch, the state converted in and out every call);
  schedule   one solve with param_schedule (k_admm_lds_pp, up to 16 iterations per launch);
  plain      the same solve without a schedule (k_admm_lds): what reading the weights by row costs.
Every process warms up untimed (one pass of its leg) and times --inner passes (wall clock between device synchronisations).
Prints one JSON line per leg and a summary line with the medians and the ratios chain / schedule and schedule / plain.
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
    import time
    import torch
    import bench
    from mgadmm import _lib as L
    from mgadmm.ADMM import geometric_ramp
    dev = torch.device("cuda", 0)
    n, _, cl, dl, info, _ = bench.build_problem("cfg2")
    y = bench.synth_y(n, args.batch, 12, 0, 0, dev)
    blk = bench.make_solver(n, cl, dl, info, dev)
    blk.check_stop = False
    names = ("rho", "rho_u", "rho_d")
    base = {nm: float(getattr(blk, nm)) for nm in names}
    sched = {nm: geometric_ramp(base[nm], args.factor, args.iters) for nm in names}

    def one_pass():
        blk._reset_history()
        if args.leg == "chain":
            blk.max_ADMM_iter = 1
            state = None
            for it in range(args.iters):
                for nm in names:
                    setattr(blk, nm, float(sched[nm][it]))
                x = blk.solve(y, warm_start=state)[0]
                state = blk.state
            return x
        blk.max_ADMM_iter = args.iters
        return blk.solve(y, return_state=False, **(dict(param_schedule=sched) if args.leg == "schedule" else {}))[0]

    times = []
    for k in range(args.inner + 1):                               # the first pass is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = one_pass()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    h = blk._solvers[(1, torch.float32)][0]
    print(json.dumps(dict(leg=args.leg, lib=L.version(), B=args.batch, iters=args.iters, unit=L.query(h, L.Q_LDS_UNIT),
                          chunk=L.query(h, L.Q_LDS_CHUNK), ms=[round(t, 3) for t in times[1:]], warmup_ms=round(times[0], 3),
                          x_checksum=float(x.double().abs().mean()))), flush=True)


def child(name, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--batch", str(args.batch), "--iters", str(args.iters),
           "--inner", str(args.inner), "--factor", str(args.factor)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"leg {name} failed with status {r.returncode}")        # nothing more is started on the GPU
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--inner", type=int, default=3, help="timed passes per process")
    ap.add_argument("--factor", type=float, default=1.03, help="growth of the three rhos per row")
    ap.add_argument("--leg-timeout", type=float, default=300.0)
    ap.add_argument("--leg", choices=["chain", "schedule", "plain"])
    ap.add_argument("--legs", default="chain,schedule,plain")
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    res = {name: child(name, args) for name in args.legs.split(",")}
    med = {k: statistics.median(v["ms"]) for k, v in res.items()}
    out = dict(summary=True, B=args.batch, iters=args.iters, factor=args.factor, median_ms={k: round(v, 3) for k, v in med.items()},
               range_ms={k: [min(v["ms"]), max(v["ms"])] for k, v in res.items()})
    if "chain" in res and "schedule" in res:
        out["chain_over_schedule"] = round(med["chain"] / med["schedule"], 3)
        out["same_x"] = res["chain"]["x_checksum"] == res["schedule"]["x_checksum"]      # the same iterations: the checksums of x agree
    if "schedule" in res and "plain" in res:
        out["schedule_over_plain"] = round(med["schedule"] / med["plain"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
