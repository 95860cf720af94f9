"""What adapting the penalties on the device costs, against the plain solve and against the host-driven chain it replaces
(DESIGN.md 3g).

    python tools/adaptive_rho_time.py [--batch 4096] [--iters 48] [--inner 3] [--every 4] [--mu 2] [--tau 2]

Problem: the tables and the synthetic inputs of bench.py's cfg2 (N = 307, T = 24, t_in = 12), B samples, a fixed count of
ADMM iterations.

Legs, one fresh process each with a time limit of its own (--leg-timeout), one after the other; a leg that fails ends the run:
  plain        (a) the solve with constant penalties (k_admm_lds, up to 16 iterations per launch);
  never16/8/4  (b) adaptive_rho with mu = 1e30 at every = 16, 8, 4: the rule never steps, so the work is the plain solve's and
               the checksum of x must equal (a)'s; what shorter launches, k_admm_lds_pp and k_lds_adapt cost;
  adaptive     (c) adaptive_rho with (--every, --mu, --tau);
  chain        (d) the loop (c) replaces: solves of --every iterations resumed with warm_start=, metrics_per_sample read on the
               host, the numpy rule applied, the per-sample penalties passed as sample_params.  Its checksum must equal (c)'s.
Every process warms up untimed (one pass of its leg) and times --inner passes (wall clock between device synchronisations).
Prints one JSON line per leg and a summary line with the medians, the ratios (b) / (a) and (d) / (c), and the checksum tests.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rho", "rho_u", "rho_d")
PAIRS = (("rho_u", 1, 2), ("rho", 3, 4), ("rho_d", 5, 6))      # penalty, MGADMM_M_PRI_*, MGADMM_M_DUAL_* of its pair


def balance(r, pri2, dual2, mu, tau, lo, hi):
    """csrc/lds_adapt.h in numpy: the same multiplications and comparisons in the same order."""
    import numpy as np
    mu, tau = np.float64(mu), np.float64(tau)
    tau_inv = np.float64(1.0) / tau
    s2 = r * r * dual2
    m2 = mu * mu
    up, down = r * tau, r * tau_inv
    up, down = np.where(up < hi, up, hi), np.where(down > lo, down, lo)
    return np.where(pri2 > m2 * s2, up, np.where(s2 > m2 * pri2, down, r))


def leg(args):
    for p in (HERE, os.path.join(HERE, "mixed-graph-admm_amd")):
        sys.path.insert(0, p)
    import time
    import numpy as np
    import torch
    import bench
    from mgadmm import _lib as L
    dev = torch.device("cuda", 0)
    n, _, cl, dl, info, _ = bench.build_problem("cfg2")
    y = bench.synth_y(n, args.batch, 12, 0, 0, dev)
    blk = bench.make_solver(n, cl, dl, info, dev)
    blk.check_stop = False
    lo, hi = 1e-6, 1e6
    ad = dict(every=args.every, mu=args.mu, tau=args.tau, rho_min=lo, rho_max=hi)
    if args.leg.startswith("never"):
        ad = dict(every=int(args.leg[5:]), mu=1e30, tau=2.0, rho_min=lo, rho_max=hi)
    steps = 0

    def one_pass():
        nonlocal steps
        blk._reset_history()
        if args.leg != "chain":
            blk.max_ADMM_iter = args.iters
            x = blk.solve(y, return_state=False, **({} if args.leg == "plain" else dict(adaptive_rho=ad)))[0]
            if blk.rho_history is not None:
                steps = int((blk.rho_history[1:] != blk.rho_history[:-1]).sum())
            return x
        w = {nm: np.full(args.batch, float(getattr(blk, nm))) for nm in NAMES}
        state, it, steps = None, 0, 0
        while it < args.iters:
            blk.max_ADMM_iter = min(args.every, args.iters - it)
            x = blk.solve(y, warm_start=state, sample_params=w, per_sample_history=True)[0]
            state, it = blk.state, it + blk.max_ADMM_iter
            if it % args.every == 0:
                m = blk.metrics_per_sample[-1]
                new = {nm: balance(w[nm], m[ip], m[idd], args.mu, args.tau, lo, hi) for nm, ip, idd in PAIRS}
                steps += sum(int((new[nm] != w[nm]).sum()) for nm in NAMES)
                w = new
        return x

    times = []
    for k in range(args.inner + 1):                               # the first pass is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = one_pass()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    h = blk._solvers[(1, torch.float32)][0]
    print(json.dumps(dict(leg=args.leg, lib=L.version(), B=args.batch, iters=args.iters, unit=L.query(h, L.Q_LDS_UNIT),
                          ms=[round(t, 3) for t in times[1:]], warmup_ms=round(times[0], 3), penalty_changes=steps,
                          x_checksum=float(x.double().abs().mean()))), flush=True)


def child(name, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--batch", str(args.batch), "--iters", str(args.iters),
           "--inner", str(args.inner), "--every", str(args.every), "--mu", str(args.mu), "--tau", str(args.tau)]
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
    ap.add_argument("--iters", type=int, default=48)
    ap.add_argument("--inner", type=int, default=3, help="timed passes per process")
    ap.add_argument("--every", type=int, default=4)
    ap.add_argument("--mu", type=float, default=2.0)
    ap.add_argument("--tau", type=float, default=2.0)
    ap.add_argument("--leg-timeout", type=float, default=300.0)
    ap.add_argument("--leg")
    ap.add_argument("--legs", default="plain,never16,never8,never4,adaptive,chain")
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    res = {name: child(name, args) for name in args.legs.split(",")}
    med = {k: statistics.median(v["ms"]) for k, v in res.items()}
    out = dict(summary=True, B=args.batch, iters=args.iters, triple=[args.every, args.mu, args.tau],
               median_ms={k: round(v, 3) for k, v in med.items()}, range_ms={k: [min(v["ms"]), max(v["ms"])] for k, v in res.items()})
    if "plain" in res:
        out["never_over_plain"] = {k: round(med[k] / med["plain"], 4) for k in res if k.startswith("never")}
        out["never_same_x"] = all(res[k]["x_checksum"] == res["plain"]["x_checksum"] for k in res if k.startswith("never"))
    if "adaptive" in res and "chain" in res:
        out["chain_over_adaptive"] = round(med["chain"] / med["adaptive"], 3)
        out["same_x"] = res["adaptive"]["x_checksum"] == res["chain"]["x_checksum"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
