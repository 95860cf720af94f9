"""CPU pre-check of the unit census (tests/test_gpu_lds_census_units.py), no GPU needed: the float64 oracle alone on the three
picks of every census row, for both units, and the conditions of the tolerance picker (lds_census.pick_admm_tol) on its
residuals -- at the test's 1 % margin and at 3 %, which shows how much room a row leaves for the float32 residuals the test
itself picks from.  A row that fails needs its own K or scales in lds_census.UNIT_OVERRIDES.

    python tools/lds_census_units_precheck.py [census row numbers]      (JOBS=n worker processes, default 8)
"""
import os, sys, time
from concurrent.futures import ProcessPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mixed-graph-admm_amd"), os.path.join(ROOT, "tests")]
import numpy as np


def one(args):
    i, unit = args
    import lds_census as lc
    from test_gpu_lds_census import _info, _inputs, _oracle, _product
    from test_gpu_sample_params import NAMES, ROWS
    r = lc.CENSUS[i]
    t0 = time.time()
    K = lc.unit_k(r)
    info = _info(r["N"], r["T"])
    y, mask = _inputs(r)
    y = (y * lc.unit_scales(r).reshape(-1, 1, 1, 1)).astype(np.float32)
    blk = _product(r, info, path="lds")
    has_phi, has_zd = r["abl"] in ("None", "DGLR"), r["abl"] != "DGLR"
    res = []
    for b in lc.unit_picks(r):
        inf = dict(info) if unit == "ps" else {nm: info[nm] * ROWS[b % 8][j] for j, nm in enumerate(NAMES)}
        o = _oracle(r, blk, inf)
        o.ADMM_tol = 0.0
        o.combined_loop(y[b:b + 1].astype(np.float64), mask=None if mask is None else mask[b:b + 1], n_iters=K)
        res.append([max(max(p), max(d)) for p, d in zip(o.hist.p_res_list, o.hist.d_res_list)])
    res = np.array(res)
    try:
        tol, n = lc.pick_admm_tol(res, K)
        gap = min(float(np.abs(np.log(row[:v] / tol)).min()) for row, v in zip(res, n))
        msg = f"OK tol {tol:.6g} n {n} gap x{np.exp(gap):.4f}"
        try:
            t2, n2 = lc.pick_admm_tol(res, K, margin=0.03)
            msg += f"; at 3 %: tol {t2:.6g} n {n2}"
        except AssertionError:
            msg += "; NONE at 3 %"
    except AssertionError as e:
        msg = f"FAIL {e}\n" + np.array2string(res, precision=4, max_line_width=250)
    return f"{lc.row_id(r)}-{unit} K={K} {r['abl']} {r['task']} B={r['B']}: {msg} ({time.time() - t0:.1f} s)"


if __name__ == "__main__":
    import lds_census as lc
    rows = [int(a) for a in sys.argv[1:]] or range(len(lc.CENSUS))
    jobs = [(i, u) for i in rows for u in lc.UNITS]
    with ProcessPoolExecutor(int(os.environ.get("JOBS", "8"))) as ex:
        for s in ex.map(one, jobs):
            print(s, flush=True)
