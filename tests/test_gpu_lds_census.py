"""Every shipped k_admm_lds instance against the float64 oracle (tests/lds_census.py: one row per instance).

For each census row:
  1. the solver takes the LDS path and reports (MGADMM_Q_LDS_INSTANCE) that it launched the row's instance (-1 before the
     first launch), and it reports the planner's geometry of the row (threads, LDS rows incl. ghosts, row stride);
  2. 6 ADMM iterations in one launch (default chunk, no stop test) on B windows; windows 0, B-1 and an interior one are
     compared with the oracle at the tolerances of the BASELINE configs (helpers.check_windows): x per sample 1e-5, every
     history list rtol 1e-3 (floor 1e-7 ||x||), CG counts +-1 (+-2 for the diagonal x solve of 'DGTV' / 'UT'); where the
     float64 count is a finite-termination count (the oracle's last step cuts ||r|| below float32 resolution: the x solve
     of a T = 12 skip-1 line graph stops after exactly 12 iterations) the bound of test_gpu_random.py for such counts,
     [ref - 1, 2 ref + 1], applies as well;
  3. x per node: the largest error of a node's time series (relative to the window's RMS node norm) at most twice the one
     of the float32 streaming path on the same windows -- a wrong entry of one table row (one hub) is diluted in the
     per-sample norm by sqrt(N), not here;
  4. the exported state (zu, zd, gamma_u, gamma_d, phi, gamma) against OracleADMM.state: zu at 1e-4 and phi at 1e-3 (the
     bounds of test_gpu_parity.py); zd and the duals, which nothing else bounds, at most twice the error the float32
     streaming path makes on the same windows and at most 1e-4 ('DGLR' leaves zd and gamma_d at their initial values:
     the same bound, and gamma_d exactly 0.1);
  5. the same solve in chunks of 4 iterations per launch (MGADMM_LDS_CHUNK=4: a launch boundary inside the run) gives
     x, state and every history list bit for bit.
"""
import math
import time

import numpy as np
import pytest
import torch

import lds_census as lc
from helpers import check_windows

pytestmark = pytest.mark.gpu

ITERS = 6
ZU_TOL, PHI_TOL = 1e-4, 1e-3           # test_gpu_parity.py: float32 zu / phi against the float64 reference
STATE_TOL, STREAM_FACTOR = 1e-4, 2.0   # zd, gamma_u, gamma_d, gamma: <= min(STATE_TOL, STREAM_FACTOR * streaming-path error);
                                       # x per node: <= STREAM_FACTOR * streaming-path error
LISTS = ("p_res_list", "d_res_list", "x_shift_list", "GLR_list", "DGTV_list", "DGLR_list", "recover_list",
         "CG_iter_x", "CG_iter_zu", "CG_iter_zd")


def _info(N, T):
    r = math.sqrt(N / T)
    return dict(rho=2 * r, rho_u=3 * r, rho_d=2 * r, mu_u=1, mu_d1=2, mu_d2=1)


def _product(r, info, **kw):
    import mgadmm
    N, T, kind = r["N"], r["T"], r["kind"]
    common = dict(ablation=r["abl"], t_in=r["t_in"], T=T, record_cg_coeffs=False, **kw)
    if kind == "physical":
        ue, ud = lc.physical_graph(N)
        return mgadmm.ADMM_algorithm({"n_nodes": N, "u_edges": ue, "u_dist": ud}, info, use_kNN=False, **common)
    cl, dl = lc.tables_for(r)
    line = kind.startswith("line")
    return mgadmm.ADMM_algorithm({"n_nodes": N}, info, use_kNN=True, k=cl.shape[1] - 1, tables=(cl, dl),
                                 use_line_graph=line, skip_connection=3 if kind == "line3" else 1, **common)


def _oracle(r, blk, info):
    from oracle import admm_oracle as orc
    cl = blk.connect_list.numpy()
    kw = dict(ablation=r["abl"], t_in=r["t_in"], T=r["T"])
    if r["kind"].startswith("line"):
        return orc.OracleADMM(cl, blk.u_ew[0].numpy(), None, info, mode="line", skip_connection=blk.skip_connection, **kw)
    mode = "physical" if r["kind"] == "physical" else "knn"
    return orc.OracleADMM(cl, blk.u_ew[0].numpy(), blk.d_ew[0].numpy(), info, mode=mode, **kw)


def _inputs(r, seed=0):
    rng = np.random.default_rng(seed)
    B, T, N, t_in = r["B"], r["T"], r["N"], r["t_in"]
    x_true = (100 + 50 * rng.random((B, T, N, 1))).astype(np.float32)
    if r["task"] == "pred":
        return x_true[:, :t_in].copy(), None
    mask = (rng.random((B, T, N, 1)) >= 0.4).astype(np.float32)
    return x_true * mask, mask


def _solve(blk, y, mask):
    blk.max_ADMM_iter = ITERS
    blk.check_stop = False
    blk._reset_history()
    x, _, _, _ = blk.solve(torch.from_numpy(y), mask=None if mask is None else torch.from_numpy(mask), per_sample_history=True)
    return dict(x=x.clone(), state={k: v.clone() for k, v in blk.state.items()},
                lists={k: [np.asarray(v) for v in getattr(blk, k)] for k in LISTS},
                dxps=np.array([np.asarray(v) for v in blk.delta_x_per_step]), mps=blk.metrics_per_sample.copy())


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _node_errors(out, xo, idx):
    """(windows, N): error of each node's time series relative to the window's RMS node norm."""
    xg = out["x"][torch.as_tensor(idx)].double().numpy()
    rms = np.sqrt((xo ** 2).sum((1, 2, 3)) / xo.shape[2])
    return np.linalg.norm(xg - xo, axis=1)[..., 0] / rms[:, None]


def _state_errors(out, o, idx):
    t = torch.as_tensor(idx)
    return {k: _rel(out["state"][k][t].double().numpy(), o.state[k]) for k in o.state if k != "x"}


@pytest.fixture
def env(monkeypatch):
    for k in ("MGADMM_LDS_TPG", "MGADMM_LDS_NOSLOTS", "MGADMM_LDS_SB", "MGADMM_LDS_RAGGED", "MGADMM_LDS_TABLE_ORDER",
              "MGADMM_LDS_CHUNK", "MGADMM_LDS_BANK_SEARCH", "MGADMM_LDS_ASYNC"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.mark.parametrize("r", lc.CENSUS, ids=lc.row_id)
def test_instance_against_the_oracle(r, env):
    from mgadmm import _lib
    t0 = time.time()
    for k, v in r["env"].items():
        env.setenv(k, v)
    info = _info(r["N"], r["T"])
    y, mask = _inputs(r)
    B = r["B"]
    idx = np.array([0, B // 2, B - 1])
    blk = _product(r, info, path="lds")
    h = blk._solver(1, torch.float32, B)[0]
    tag = f"{r['expect']} N={r['N']} T={r['T']} t_in={r['t_in']} {r['kind']} {r['abl']} {r['task']} B={B}"
    assert _lib.query(h, _lib.Q_LDS_INSTANCE) == -1 and _lib.lds_instance(h) is None, tag      # no launch yet
    out = _solve(blk, y, mask)
    assert blk._solvers[(1, torch.float32)][0].value == h.value                                 # the same solver
    assert _lib.lib.mgadmm_solver_path(h, B) == _lib.PATH_LDS, tag
    assert _lib.lds_instance(h) == r["expect"], tag
    nth, rows, ts, ghosts = lc.geometry(r)
    geo = [_lib.query(h, q) for q in (_lib.Q_LDS_THREADS, _lib.Q_LDS_ROWS, _lib.Q_LDS_ROW_STRIDE)]
    assert geo == [nth, rows, ts], (tag, "threads / rows / stride", geo, (nth, rows, ts), f"{ghosts} ghosts")
    assert _lib.query(h, _lib.Q_LDS_CHUNK) >= ITERS                     # the 6 iterations ran in one launch

    # the float64 oracle on three windows; the float32 streaming path on the same problem (state error scale)
    o = _oracle(r, blk, info)
    xo = o.combined_loop(y[idx].astype(np.float64), mask=None if mask is None else mask[idx], n_iters=ITERS)
    err = _state_errors(out, o, idx)
    blk_s = _product(r, info, path="stream")
    ref = _solve(blk_s, y, mask)
    blk_s.close()
    serr = _state_errors(ref, o, idx)
    node, snode = _node_errors(out, xo, idx), _node_errors(ref, xo, idx)
    print(f"\n[census] {tag}: x per node LDS / stream {node.max():.2e}/{snode.max():.2e} "
          f"(node {np.unravel_index(np.argmax(node), node.shape)[1]}); "
          "state LDS / stream: " + ", ".join(f"{k} {err[k]:.2e}/{serr[k]:.2e}" for k in err)
          + "; CG x count off by (LDS / stream): " + "/".join(
              str(int(np.abs(np.stack(d["lists"]["CG_iter_x"])[:, idx] - np.array(o.hist.CG_iter_x).reshape(ITERS, -1)).max()))
              for d in (out, ref)))

    check_windows(tag, blk, out["x"], idx, o, xo, abl=r["abl"], finite_termination_rule=True)
    blk.close()
    assert node.max() <= STREAM_FACTOR * snode.max(), (tag, "x per node", node.max(), snode.max())
    assert err["zu"] <= ZU_TOL, (tag, "zu", err["zu"])
    if "phi" in err:
        assert err["phi"] <= PHI_TOL, (tag, "phi", err["phi"])
    for k in ("zd", "gamma_u", "gamma_d", "gamma"):
        if k in err:
            bound = min(STATE_TOL, STREAM_FACTOR * serr[k])
            assert err[k] <= bound, (tag, k, err[k], serr[k])
    if r["abl"] == "DGLR":
        assert (out["state"]["gamma_d"] == np.float32(0.1)).all(), tag

    # a launch boundary every 4 iterations: the same bits
    env.setenv("MGADMM_LDS_CHUNK", "4")
    blk4 = _product(r, info, path="lds")
    out4 = _solve(blk4, y, mask)
    h4 = blk4._solvers[(1, torch.float32)][0]
    assert _lib.query(h4, _lib.Q_LDS_CHUNK) == 4 and _lib.lds_instance(h4) == r["expect"]
    blk4.close()
    assert torch.equal(out["x"], out4["x"]), tag
    assert out["state"].keys() == out4["state"].keys()
    for k in out["state"]:
        assert torch.equal(out["state"][k], out4["state"][k]), (tag, "state." + k)
    for k in LISTS:
        assert len(out["lists"][k]) == len(out4["lists"][k])
        for a, b in zip(out["lists"][k], out4["lists"][k]):
            np.testing.assert_array_equal(a, b, err_msg=f"{tag} {k}")
    np.testing.assert_array_equal(out["dxps"], out4["dxps"])
    np.testing.assert_array_equal(out["mps"], out4["mps"])
    print(f"[census] {tag}: {time.time() - t0:.1f} s")
