"""Every streaming-path kernel class against the float64 oracle (tests/stream_census.py: one row per problem).

For each census row, with path="stream":
  1. operators Lu, Ldr, Ldr_T, cLdr, Ln, phi_direct and the left-hand sides LHS_x (also with a mask), LHS_zu, LHS_zd on all B
     samples of random normal input: relative error 2e-6 (float32) / 1e-12 (float64), the tolerances of test_gpu_random.py /
     test_gpu_parity.py, and per node -- the largest error of a node's time series relative to the sample's RMS node norm --
     the same bound times sqrt(N): one bad table row is not diluted by the other N - 1;
  2. one CG solve per left-hand side on all B systems, 4 of them against the oracle: 1e-5 with counts +-1 (float32), 1e-9 with
     equal counts (float64); the same solves under MGADMM_FOLD=0: identical counts, x to 1e-6.  Two exceptions to +-1, both
     for float64 counts that are finite-termination counts float32 cannot reproduce: the diagonal x system of 'DGTV' / 'UT'
     (two distinct eigenvalues: 2 iterations in float64, 4 in float32 on every such row) gets the +-2 that check_solve of
     test_gpu_parity.py and helpers.check_windows give that solve; the two float32 rows on the skip-1 line graph (float64 4,
     float32 7 and 8 at T = 4) get the bound of test_gpu_random.py for line graphs, [ref - 1, 2 ref + 1], where the oracle's
     own last step shows the termination (helpers.finite_termination).  The same two rows pass finite_termination_rule to
     check_windows in step 3 (x counts off by 4 there); every other row runs it at its defaults;
  3. a 4-iteration solve (no stop test, per-sample history), windows 0, B/2 and B-1 against the oracle at the BASELINE
     tolerances of helpers.check_windows (float64: 1e-9 / 1e-7 / slack 0);
  4. rows on k_tile / k_cldr: x per node on those windows at most STREAM_FACTOR = 2 times the error of the plain row kernels
     (MGADMM_TILE=0, natural node order) -- the same arithmetic in another summation order, as in test_gpu_lds_census.py;
  5. the solve again on the same solver: x and every history list bit for bit;
  6. the solver launched exactly the instances the row names (MGADMM_Q_STREAM_KEYS), none of the UNREACHABLE table, and
     reports the row's MGADMM_Q_CLDR_SLOTS and MGADMM_Q_TILE_ROWS.
"""
import math
import re
import time

import numpy as np
import pytest
import torch

import stream_census as sc
import lds_census as lc
from helpers import F32_EPS, check_windows, rel

pytestmark = pytest.mark.gpu

ITERS = 4
STREAM_FACTOR = 2.0
LISTS = ("p_res_list", "d_res_list", "x_shift_list", "GLR_list", "DGTV_list", "DGLR_list", "recover_list",
         "CG_iter_x", "CG_iter_zu", "CG_iter_zd")
SWITCHES = ("MGADMM_TILE", "MGADMM_TILE_R", "MGADMM_FUSED", "MGADMM_FOLD", "MGADMM_FOLD_LU", "MGADMM_SWEEP_REV", "MGADMM_CLDR_ORDER",
            "MGADMM_CLDR_GEOM", "MGADMM_CLDR_ROWS", "MGADMM_WANT_BLOCKS", "MGADMM_TILE_STATS")


def _info(N, T):
    r = math.sqrt(N / T)
    return dict(rho=2 * r, rho_u=3 * r, rho_d=2 * r, mu_u=1, mu_d1=2, mu_d2=1)


def _product(r, info, reorder=None):
    import mgadmm
    N, T, kind = r["N"], r["T"], r["graph"][0]
    dt = torch.float32 if r["dtype"] == "f32" else torch.float64
    reorder = r["reorder"] if reorder is None else reorder
    common = dict(ablation=r["abl"], t_in=r["t_in"], T=T, record_cg_coeffs=False, compute_dtype=dt, path="stream",
                  reorder="cluster" if reorder else 0)
    if kind == "physical":
        ue, ud = lc.physical_graph(N)
        return mgadmm.ADMM_algorithm({"n_nodes": N, "u_edges": ue, "u_dist": ud}, info, use_kNN=False, **common)
    cl, dl = sc.tables_for(r)
    return mgadmm.ADMM_algorithm({"n_nodes": N}, info, use_kNN=True, k=cl.shape[1] - 1, tables=(cl, dl),
                                 use_line_graph=kind in ("line", "skip3"), skip_connection=3 if kind == "skip3" else 1, **common)


def _oracle(r, blk, info):
    from oracle import admm_oracle as orc
    cl = blk.connect_list.numpy()
    kw = dict(ablation=r["abl"], t_in=r["t_in"], T=r["T"])
    kind = r["graph"][0]
    if kind in ("line", "skip3"):
        return orc.OracleADMM(cl, blk.u_ew[0].numpy(), None, info, mode="line", skip_connection=blk.skip_connection, **kw)
    return orc.OracleADMM(cl, blk.u_ew[0].numpy(), blk.d_ew[0].numpy(), info, mode="physical" if kind == "physical" else "knn", **kw)


def _node_error(got, ref):
    """Largest error of a node's time series relative to its sample's RMS node norm; got, ref: (b, T, N, 1)."""
    got = got.double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    rms = np.sqrt((ref ** 2).sum((1, 2, 3)) / ref.shape[2])
    return float((np.linalg.norm(got - ref, axis=1)[..., 0] / rms[:, None]).max())


def _solve(blk, y, mask, dt):
    blk.max_ADMM_iter = ITERS
    blk.check_stop = False
    blk._reset_history()
    x = blk.solve(torch.from_numpy(y).to(dt), mask=None if mask is None else torch.from_numpy(mask).to(dt), per_sample_history=True)[0]
    return dict(x=x.clone(), lists={k: [np.asarray(v) for v in getattr(blk, k)] for k in LISTS},
                dxps=np.array([np.asarray(v) for v in blk.delta_x_per_step]), mps=blk.metrics_per_sample.copy())


@pytest.fixture
def env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.mark.parametrize("r", sc.CENSUS, ids=sc.row_id)
def test_problem_against_the_oracle(r, env):
    from mgadmm import _lib
    t0 = time.time()
    for k, v in r["env"].items():
        env.setenv(k, v)
    f32 = r["dtype"] == "f32"
    dt = torch.float32 if f32 else torch.float64
    N, T, B, t_in = r["N"], r["T"], r["B"], r["t_in"]
    tag = f"{r['name']} N={N} T={T} {r['graph']} {r['abl']} {r['task']} B={B} {r['env']}"
    info = _info(N, T)
    rng = np.random.default_rng(3)
    blk = _product(r, info)
    o = _oracle(r, blk, info)
    T_ = lambda a: None if a is None else torch.from_numpy(a).to(dt)

    # ---- 1. operators and left-hand sides, all B samples
    tol = 2e-6 if f32 else 1e-12
    x = rng.standard_normal((B, T, N, 1)).astype(np.float32)
    gam = rng.standard_normal((B, T, N, 1)).astype(np.float32)
    m01 = (rng.random((B, T, N, 1)) >= 0.4).astype(np.float32)
    x64, xt = x.astype(np.float64), T_(x)
    pairs = [("Lu", blk.apply_op_Lu(xt), o.apply_op_Lu(x64)), ("Ldr", blk.apply_op_Ldr(xt), o.apply_op_Ldr(x64)),
             ("Ldr_T", blk.apply_op_Ldr_T(xt), o.apply_op_Ldr_T(x64)), ("cLdr", blk.apply_op_cLdr(xt), o.apply_op_cLdr(x64)),
             ("Ln", blk.apply_op_Ln(xt), o.apply_op_Ln(x64)),
             ("phi_direct", blk.phi_direct(xt, T_(gam)), o.phi_direct(x64, gam.astype(np.float64))),
             ("LHS_x", blk.LHS_x(xt), o.LHS_x(x64)), ("LHS_x mask", blk.LHS_x(xt, T_(m01)), o.LHS_x(x64, mask=m01.astype(np.float64))),
             ("LHS_zu", blk.LHS_zu(xt), o.LHS_zu(x64))]
    if r["abl"] != "DGLR":
        pairs.append(("LHS_zd", blk.LHS_zd(xt), o.LHS_zd(x64)))
    h = blk._solvers[(1, dt)][0]
    worst = {}
    for nm, got, ref in pairs:
        ref = np.asarray(ref, dtype=np.float64)
        e, en = rel(got, ref), _node_error(got, ref)
        worst[nm] = (e, en)
        assert e < tol, (tag, nm, e)
        assert en < tol * math.sqrt(N), (tag, nm, "per node", en)

    # ---- 2. CG, 4 systems against the oracle; MGADMM_FOLD=0 on a second solver
    idx4 = np.unique(np.array([0, B // 3, 2 * B // 3, B - 1]))
    rhs = (rng.standard_normal((B, T, N, 1)) * np.logspace(-1, 1, B).reshape(B, 1, 1, 1)).astype(np.float32)
    mask_cg = m01 if r["task"] == "mask" else None
    solves = [("x", "LHS_x", dict(mask=T_(mask_cg)) if mask_cg is not None else {}), ("zu", "LHS_zu", {})]
    if r["abl"] != "DGLR":
        solves.append(("zd", "LHS_zd", {}))
    cg = {}
    for nm, fn, kw in solves:
        xs, it, _, _ = blk.CG_solver(getattr(blk, fn), T_(rhs), xt, **kw)
        okw = dict(mask=mask_cg[idx4].astype(np.float64)) if kw else {}
        xo, ito, _, beo = o.CG_solver(getattr(o, fn), rhs[idx4].astype(np.float64), x64[idx4], **okw)
        it, ito = np.asarray(it).reshape(-1), np.asarray(ito).reshape(-1)
        cg[nm] = (xs, it)
        e = rel(xs[torch.as_tensor(idx4)], xo)
        fin = np.array([k > 0 and np.sqrt(beo[k - 1, j]) < F32_EPS for j, k in enumerate(ito)])      # helpers.finite_termination
        print(f"\n[stream census] {r['name']} CG {nm}: rel {e:.2e}, counts {it[idx4].tolist()} oracle {ito.tolist()} finite termination {fin.tolist()}")
        assert e < (1e-5 if f32 else 1e-9), (tag, "CG", nm, e)
        assert (ito > 0).all(), (tag, "CG", nm, "the oracle did not converge", ito)
        if f32:
            # +-1; the diagonal x system of 'DGTV' / 'UT' +-2 (check_solve of test_gpu_parity.py, helpers.check_windows); on
            # the line graphs alone, where the oracle's own last step marks finite termination, test_gpu_random.py's
            # [ref - 1, 2 ref + 1]
            ok = np.abs(it[idx4] - ito) <= (2 if nm == "x" and r["abl"] in ("DGTV", "UT") else 1)
            if r["graph"][0] == "line":
                ok |= fin & (it[idx4] >= ito - 1) & (it[idx4] <= 2 * ito + 1)
            assert ok.all(), (tag, "CG", nm, "counts", it[idx4], ito, fin)
        else:
            assert (it[idx4] == ito).all(), (tag, "CG", nm, "counts", it[idx4], ito)
    got = _lib.stream_instances(h)
    want = sc.expected(r, phases=("ops", "cg"))
    assert got == want, (tag, dict(missing=sorted(want - got), extra=sorted(got - want)))

    env.setenv("MGADMM_FOLD", "0")
    blk0 = _product(r, info)
    for nm, fn, kw in solves:
        xs0, it0, _, _ = blk0.CG_solver(getattr(blk0, fn), T_(rhs), xt, **kw)
        assert np.array_equal(np.asarray(it0).reshape(-1), cg[nm][1]), (tag, "MGADMM_FOLD=0 counts", nm)
        assert rel(xs0, cg[nm][0]) < 1e-6, (tag, "MGADMM_FOLD=0", nm)
    got0 = _lib.stream_instances(blk0._solvers[(1, dt)][0])
    want0 = sc.expected(r, phases=("cg",), env=dict(r["env"], MGADMM_FOLD="0"))
    assert got0 == want0, (tag, "MGADMM_FOLD=0", dict(missing=sorted(want0 - got0), extra=sorted(got0 - want0)))
    blk0.close()
    env.delenv("MGADMM_FOLD")
    for k, v in r["env"].items():
        env.setenv(k, v)

    # ---- 3. the ADMM loop on windows 0, B/2, B-1
    idx = np.unique(np.array([0, B // 2, B - 1]))
    x_true = (100 + 50 * rng.random((B, T, N, 1))).astype(np.float32)
    if r["task"] == "pred":
        y, mask = x_true[:, :t_in].copy(), None
    else:
        # 40 % of the entries hidden, but three steps of every node observed: the interpolation of the initial guess needs two
        mask = (rng.random((B, T, N, 1)) >= 0.4).astype(np.float32)
        for j in range(3):
            mask[:, (np.arange(N) + j * (T // 3 or 1)) % T, np.arange(N)] = 1.0
        y = x_true * mask
    out = _solve(blk, y, mask, dt)
    assert blk._solvers[(1, dt)][0].value == h.value                                 # the same solver throughout
    xo = o.combined_loop(y[idx].astype(np.float64), mask=None if mask is None else mask[idx].astype(np.float64), n_iters=ITERS)
    if f32:
        # (skip-1 line graph: the x solve has a handful of distinct eigenvalues and the float64 count is a finite-termination
        # count; test_gpu_random.py bounds the float32 count of such solves by [ref - 1, 2 ref + 1], check_windows where the
        # oracle's last step shows it)
        check_windows(tag, blk, out["x"], idx, o, xo, abl=r["abl"], finite_termination_rule=r["graph"][0] == "line")
    else:
        check_windows(tag, blk, out["x"], idx, o, xo, xtol=1e-9, htol=1e-7, slack=0, abl=r["abl"])

    # ---- 6. what ran
    got = _lib.stream_instances(h)
    want = sc.expected(r, phases=("ops", "cg", "solve"))
    assert got == want, (tag, dict(missing=sorted(want - got), extra=sorted(got - want)))
    for pat, why in sc.UNREACHABLE:
        assert not [n for n in got if re.fullmatch(pat, n)], (tag, "launched an UNREACHABLE instance", pat)
    assert _lib.query(h, _lib.Q_CLDR_SLOTS) == r["slots"], (tag, "Q_CLDR_SLOTS", _lib.query(h, _lib.Q_CLDR_SLOTS))
    assert _lib.query(h, _lib.Q_TILE_ROWS) == r["tile_rows"], (tag, "Q_TILE_ROWS", _lib.query(h, _lib.Q_TILE_ROWS))
    n_keys = _lib.query(h, _lib.Q_STREAM_KEYS)
    assert n_keys == len(got)
    with pytest.raises(_lib.MgadmmError):
        _lib.query(h, _lib.Q_STREAM_KEY0 + n_keys)

    # ---- 5. again on the same solver: the same bits
    out2 = _solve(blk, y, mask, dt)
    assert torch.equal(out["x"], out2["x"]), tag
    for k in LISTS:
        assert len(out["lists"][k]) == len(out2["lists"][k])
        for a, b in zip(out["lists"][k], out2["lists"][k]):
            np.testing.assert_array_equal(a, b, err_msg=f"{tag} {k}")
    np.testing.assert_array_equal(out["dxps"], out2["dxps"])
    np.testing.assert_array_equal(out["mps"], out2["mps"])
    assert _lib.stream_instances(h) == got
    blk.close()

    # ---- 4. k_tile / k_cldr rows: x per node against the plain row kernels on the same windows
    node = _node_error(out["x"][torch.as_tensor(idx)], xo)
    if r["tile_rows"]:
        env.setenv("MGADMM_TILE", "0")
        blk_p = _product(r, info, reorder=False)
        ref = _solve(blk_p, y, mask, dt)
        names = _lib.stream_instances(blk_p._solvers[(1, dt)][0])
        blk_p.close()
        assert names and all(n.startswith("k_rows<") for n in names), (tag, sorted(names))
        pnode = _node_error(ref["x"][torch.as_tensor(idx)], xo)
        print(f"[stream census] {r['name']}: x per node {node:.2e}, plain row kernels {pnode:.2e}")
        assert node <= STREAM_FACTOR * pnode, (tag, "x per node", node, pnode)
    print(f"[stream census] {r['name']}: ops " + ", ".join(f"{k} {v[0]:.1e}/{v[1]:.1e}" for k, v in worst.items())
          + f"; x per node {node:.2e}; {time.time() - t0:.1f} s")
