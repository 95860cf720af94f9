"""Time in which no k_admm_lds launch runs, from one rocprofv3 --kernel-trace run of `bench.py --steps K` (CHUNKS schedule).

    python tools/launch_gaps.py <trace dir> [--steps K] [--chunk J] [--rows]

--rows also lists every kernel of the solve: start relative to the solve's first kernel, duration.

The solves of the run are told apart by their k_init_lds launch; the LAST solve (the timed one) is reported.  Per launch c:
its duration, the gap to the start of launch c + 1 (period minus duration) and the backlog = metric kernels of the chunks
before c that had not STARTED when launch c ended (the metric kernels of chunk c itself cannot start before that).  Then the
tail: end of the last launch to the end of the last metric kernel of the solve.  A metric kernel is any kernel of the solve
whose name starts with k_dxps, k_batch_metrics or k_lds_metric.
"""
import csv, glob, sys

METRIC = ("k_dxps", "k_batch_metrics", "k_lds_metric")


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--anchor", default="k_admm_lds")
    ap.add_argument("--steps", type=int, default=50, help="ADMM iterations of the traced solve")
    ap.add_argument("--chunk", type=int, default=16, help="iterations per launch (MGADMM_LDS_CHUNK)")
    ap.add_argument("--rows", action="store_true")
    a = ap.parse_args()
    anchor, steps, chunk, rows_too = a.anchor, a.steps, a.chunk, a.rows
    f = glob.glob(a.trace + '/**/*kernel_trace.csv', recursive=True)[0]
    rows = [(int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name'].replace('void ', '')) for r in csv.DictReader(open(f))]
    rows.sort()
    inits = [i for i, r in enumerate(rows) if r[2].startswith("k_init_lds")]
    solve = rows[inits[-1]:]
    anchors = [r for r in solve if anchor in r[2]]
    metric = [r for r in solve if r[2].startswith(METRIC)]
    names = sorted({r[2].split('(')[0] for r in metric})
    t0 = solve[0][0]                                                         # (kernels the caller runs after the solve do not count)
    t1 = max(max(r[1] for r in anchors), max(r[1] for r in metric))
    print(f"# last solve of the trace: {len(anchors)} launches of '{anchor}', {len(metric)} metric kernels ({', '.join(names)}), "
          f"first kernel start to last kernel end {(t1 - t0) / 1e3:.1f} us")
    print(f"{'launch':>6s} {'duration_us':>12s} {'gap_to_next_us':>15s} {'metric_started_by_end':>22s} {'started_during_gap':>19s}")
    gaps = 0.0
    for c, a in enumerate(anchors):
        nxt = anchors[c + 1][0] if c + 1 < len(anchors) else None
        gap = (nxt - a[1]) / 1e3 if nxt is not None else float('nan')
        started = sum(1 for m in metric if m[0] < a[1])
        in_gap = sum(1 for m in metric if a[1] <= m[0] < nxt) if nxt is not None else 0
        if nxt is not None:
            gaps += gap
        print(f"{c:6d} {(a[1] - a[0]) / 1e3:12.1f} {gap:15.1f} {started:22d} {in_gap:19d}")
    last_metric_end = max(m[1] for m in metric)
    tail = (last_metric_end - anchors[-1][1]) / 1e3
    busy = sum(m[1] - m[0] for m in metric) / 1e3
    print(f"gaps between launches, summed: {gaps:.1f} us")
    print(f"tail (end of the last launch to the end of the last metric kernel): {tail:.1f} us")
    print(f"gaps + tail: {gaps + tail:.1f} us = {100 * (gaps + tail) / ((t1 - t0) / 1e3):.2f} % of the solve")
    print(f"metric kernels, sum of durations: {busy:.1f} us; the longest one {max(m[1] - m[0] for m in metric) / 1e3:.1f} us")
    # the metric kernels run in stream order, n per iteration, those of chunk c after launch c: what the chunks before launch c
    # issued, less what had started when it ended
    its = [min(chunk, steps - c * chunk) for c in range(len(anchors))]
    per_it = len(metric) / float(steps)
    print(f"backlog at the end of each launch (metric kernels of earlier chunks not yet started; {per_it:g} per iteration, launches of {its} iterations):")
    for c, a in enumerate(anchors):
        started = sum(1 for m in metric if m[0] < a[1])
        print(f"  launch {c}: {per_it * sum(its[:c]) - started:.0f}")
    if rows_too:
        print(f"{'kernel':50s} {'start_us':>14s} {'duration_us':>12s}")
        for r in solve:
            if r[1] <= t1:
                print(f"{r[2][:48]:50s} {(r[0] - t0) / 1e3:14.1f} {(r[1] - r[0]) / 1e3:12.1f}")


if __name__ == '__main__':
    main()
