"""Time-varying edge weights on the streaming path (``ADMM_algorithm(time_varying=True)``, mgadmm_graph_set_time_weights, the row
kernel k_rows_tv) against the reference's own output on such tables (tests/golden/g11_time_varying.npz) and against the float64
restatement tests/tv_oracle.py, which tests/test_tv_oracle_golden.py pins against the same fixture.

Bounds: those of tests/test_gpu_parity.py -- operators float64 rel < 1e-13, float32 rel < 2e-6; solves float64 rel <= 1e-10 on
vectors with identical CG counts, float32 ||x - x_ref|| / ||x_ref|| <= 1e-5 and histories rel <= 1e-3 (check_solve, check_windows)."""
import numpy as np
import pytest
import torch

import tv_cases as tc
from conftest import load_golden
from helpers import check_windows, rel
from test_gpu_parity import check_solve

pytestmark = pytest.mark.gpu

MODES = ("knn", "physical")
OP_TOL = {torch.float64: 1e-13, torch.float32: 2e-6}


def T_(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def test_fixture_graph_reaches_every_branch_of_the_row_kernel():
    """The tail loop (a W_d^T row longer than the widest window), ragged rows, and both gather windows."""
    lu, ld, lt = tc.row_lengths("knn")
    assert lt.max() > 6                       # Ldr_T in kNN mode: rows past GW = 6 run the tail loop
    assert lu.max() <= 4 and (ld == 5).all()  # W_u rows: GW 4; W_d rows of 5: GW 6
    pu, pd_, _ = tc.row_lengths("physical")
    k = tc.g11()["physical_cl"].shape[1] - 1
    assert pu.min() < k and len(set(pu.tolist())) > 1      # a node with fewer than k neighbours: ragged rows


# ------------------------------------------------------------------ 1. operators and left-hand sides
@pytest.mark.parametrize("dt,B", [(torch.float32, 3), (torch.float32, 100), (torch.float32, 200), (torch.float64, 3), (torch.float64, 100)])
@pytest.mark.parametrize("T", [2, 3, 4])
def test_operators_and_left_hand_sides(T, dt, B):
    """Every VEC of either scalar type (B = 3 / 100 / 200), T = 2 (W_d has one slice) .. 4, both node orders, both modes, quirk Q1
    on and off, against the restatement on random data."""
    rng = np.random.default_rng(100 * T + B)
    x = rng.standard_normal((B, T, 30, 1))
    m = (rng.random((B, T, 30, 1)) >= 0.4).astype(np.float64)
    info, tol = tc.info_ops(), OP_TOL[dt]
    for mode in MODES:
        for bc in (True, False):
            o = tc.make_tv_oracle(mode, T, 1, info, bug_compat=bc)
            for reorder in (0, 2):
                blk = tc.make_tv_product(mode, T, 1, info, compute_dtype=dt, bug_compat=bc, reorder=reorder)
                for nm in ("Lu", "Ldr", "Ldr_T", "cLdr"):
                    got = getattr(blk, "apply_op_" + nm)(T_(x, dt))
                    assert rel(got, getattr(o, "apply_op_" + nm)(x)) < tol, (mode, nm, reorder, bc)
                assert rel(blk.LHS_x(T_(x, dt), mask=T_(m, dt)), o.LHS_x(x, mask=m)) < tol, (mode, reorder, bc)
                assert rel(blk.LHS_x(T_(x, dt)), o.LHS_x(x)) < tol
                assert rel(blk.LHS_zu(T_(x, dt)), o.LHS_zu(x)) < tol
                assert rel(blk.LHS_zd(T_(x, dt)), o.LHS_zd(x)) < tol
                blk.close()


@pytest.mark.parametrize("mode", MODES)
def test_dense_matrices_of_the_reference(mode):
    """The reference's dense matrices at T = 4 (a batch of 120 unit vectors: VEC 2), float64."""
    g = tc.g11()
    T, t_in, n = int(g["T_ops"]), int(g["t_in_ops"]), int(g["n"])
    size = T * n
    eye = torch.eye(size, dtype=torch.float64).reshape(size, T, n, 1)
    G = lambda nm: g[f"ops/{mode}/{nm}"]
    for reorder in (0, 2):
        blk = tc.make_tv_product(mode, T, t_in, tc.info_ops(), compute_dtype=torch.float64, reorder=reorder)
        for nm in ("Lu", "Ldr", "Ldr_T", "cLdr"):
            D = getattr(blk, "apply_op_" + nm)(eye).reshape(size, size).T
            assert rel(D, G(nm)) < 1e-13, (nm, reorder)
        for nm in ("LHS_x", "LHS_zu", "LHS_zd"):
            assert rel(getattr(blk, nm)(eye).reshape(size, size).T, G(nm)) < 1e-13, (nm, reorder)
        mk = T_(g["ops/mask"]).expand(size, -1, -1, -1).contiguous()
        assert rel(blk.LHS_x(eye, mask=mk).reshape(size, size).T, G("LHS_x_mask")) < 1e-13
        blk.close()


def test_two_channels_fold_into_nodes():
    T, info = 3, tc.info_ops()
    x = np.random.default_rng(5).standard_normal((3, T, 30, 2))
    for mode in MODES:
        o = tc.make_tv_oracle(mode, T, 1, info)
        blk = tc.make_tv_product(mode, T, 1, info, compute_dtype=torch.float64)
        for nm in ("Lu", "Ldr", "Ldr_T", "cLdr"):
            assert rel(getattr(blk, "apply_op_" + nm)(T_(x)), getattr(o, "apply_op_" + nm)(x)) < 1e-13, (mode, nm)
        assert rel(blk.LHS_x(T_(x)), o.LHS_x(x)) < 1e-13
        blk.close()


def test_cg_matches_the_reference():
    g = tc.g11()
    T, t_in = int(g["T_ops"]), int(g["t_in_ops"])
    rhs, x0, m = g["cg/rhs"], g["cg/x0"], g["ops/mask"]
    for mode in MODES:
        blk = tc.make_tv_product(mode, T, t_in, tc.info_ops(), compute_dtype=torch.float64)
        for nm, fn, kw in (("x", blk.LHS_x, {}), ("xmask", blk.LHS_x, {"mask": T_(m)}), ("zu", blk.LHS_zu, {}), ("zd", blk.LHS_zd, {})):
            x, it, al, be = blk.CG_solver(fn, T_(rhs), T_(x0), **kw)
            pre = f"cg/{mode}/{nm}_"
            assert it == int(g[pre + "iters"]), (mode, nm)
            assert rel(x, g[pre + "x"]) < 1e-11
            np.testing.assert_allclose(al.numpy(), g[pre + "alpha"], rtol=2e-7)
            np.testing.assert_allclose(be.numpy(), g[pre + "beta"], rtol=2e-7, atol=1e-12)
        blk.close()


# ------------------------------------------------------------------ 2. repeats through the new kernel
def _solve_all(blk, y, mask):
    x, _, _, hist = blk.solve(y, mask=mask)
    vecs = dict(blk.state)
    assert set(vecs) == {"x", "zu", "zd", "phi", "gamma", "gamma_u", "gamma_d"} and torch.equal(vecs["x"], x)
    return vecs, hist


def _assert_bitwise(a, b, what):
    if isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), what
        for i, (p, q) in enumerate(zip(a, b)):
            _assert_bitwise(p, q, f"{what}[{i}]")
    else:
        a, b = (t.numpy() if torch.is_tensor(t) else np.asarray(t) for t in (a, b))
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), what


@pytest.mark.parametrize("dt,stop", [(torch.float32, False), (torch.float64, False), (torch.float32, True)])
def test_equal_slices_through_k_rows_tv_equal_the_time_invariant_rows(dt, stop, monkeypatch):
    """Tables of equal slices kept on the per-slice path (MGADMM_TV_KEEP=1) against the same instance built time-invariant under
    MGADMM_TILE=0, both on the streaming path in the cluster order: the same plan, the same products in the same order, so x, the
    six state vectors, every history list and the CG counts are equal bit for bit."""
    meta = load_golden("g4_meta.npz")
    T, t_in = 24, 12
    B = 5
    rng = np.random.default_rng(3)
    y = T_(meta["x_true"][:, :t_in] * (1 + 0.05 * rng.standard_normal((B, t_in, 30, 1))), dt)
    cl, u, d = tc.tables("knn", T)
    u_rep, d_rep = np.repeat(u[3:4], T, 0), np.repeat(d[5:6], T - 1, 0)
    runs = []
    for tv in (True, False):
        monkeypatch.setenv("MGADMM_TILE", "0")
        if tv:
            monkeypatch.setenv("MGADMM_TV_KEEP", "1")
        else:
            monkeypatch.delenv("MGADMM_TV_KEEP", raising=False)
        blk = tc.make_tv_product("knn", T, t_in, tc.info_solve(), u_ew=u_rep, d_ew=d_rep, time_varying=tv, compute_dtype=dt,
                                 path="stream", reorder="cluster")
        blk.check_stop = stop
        blk.max_ADMM_iter = 30 if stop else 6
        blk.ADMM_tol = 60.0 if stop else blk.ADMM_tol      # loose: the test is live, whichever iteration it passes at
        vecs, hist = _solve_all(blk, y, None)
        from mgadmm import _lib
        h = blk._solvers[(1, dt)][0]
        assert blk._graphs[1][0].time_varying == tv and _lib.query(h, _lib.Q_LDS_OK) == (0 if tv or dt == torch.float64 else 1)
        runs.append((vecs, hist, len(blk.p_res_list)))
        blk.close()
    (va, ha, na), (vb, hb, nb) = runs
    assert na == nb and (na == 6 if not stop else 1 <= na <= 30)
    print(f"\n[tv bitwise] {dt} stop={stop}: {na} iterations")
    for nm in va:
        assert torch.equal(va[nm], vb[nm]), nm
    assert set(ha) == set(hb)
    for nm in ha:
        _assert_bitwise(ha[nm], hb[nm], nm)


# ------------------------------------------------------------------ 3. solves against the reference
@pytest.mark.parametrize("task", ["pred", "mask"])
@pytest.mark.parametrize("mode", MODES)
def test_solves_against_the_reference(mode, task):
    from helpers import case_inputs
    g, meta = tc.g11(), load_golden("g4_meta.npz")
    key = f"{mode}-None-{task}-f64-10"
    G = lambda f: g[f"{key}/{f}"]
    for dt, xtol, htol, slack in ((torch.float64, 1e-10, 1e-8, 0), (torch.float32, 1e-5, 1e-3, 1)):
        y, mask = case_inputs(meta, task, np.float64)
        blk = tc.make_tv_product(mode, 24, 12, tc.info_solve(), compute_dtype=dt)
        blk.max_ADMM_iter = 10
        x, (zu, zd), phi, hist = blk.solve(torch.from_numpy(y), mask=torch.from_numpy(mask) if mask is not None else None)
        check_solve(blk, key, G, "None", x, xtol, htol, slack)
        if dt == torch.float64:
            assert rel(zu, G("zu")) < 1e-10 and rel(zd, G("zd")) < 1e-10 and rel(phi, G("phi")) < 1e-9
        blk.close()


# ------------------------------------------------------------------ 3b. batched solve
@pytest.fixture(scope="module")
def batch100():
    """B = 100 random samples and the restatement's solve of them (5 iterations), computed once."""
    rng = np.random.default_rng(17)
    B = 100
    y = 100 + 50 * rng.standard_normal((B, 12, 30, 1))
    o = tc.make_tv_oracle("knn", 24, 12, tc.info_solve())
    xo = o.combined_loop(y, n_iters=5)
    return y, o, xo


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_batched_solve_against_the_restatement(batch100, dt):
    y, o, xo = batch100
    B = y.shape[0]
    blk = tc.make_tv_product("knn", 24, 12, tc.info_solve(), compute_dtype=dt)
    blk.max_ADMM_iter, blk.check_stop = 5, False
    x, _, _, _ = blk.solve(T_(y), per_sample_history=True)
    if dt == torch.float64:
        err = np.linalg.norm((x.numpy() - xo).reshape(B, -1), axis=1) / np.linalg.norm(xo.reshape(B, -1), axis=1)
        assert err.max() <= 1e-10
        check_windows("tv-f64", blk, x, np.arange(B), o, xo, xtol=1e-10, htol=1e-8, slack=0)
    else:
        check_windows("tv-f32", blk, x, np.arange(B), o, xo, xtol=1e-5, htol=1e-3, slack=1)
    blk.close()


# ------------------------------------------------------------------ 4. refusals and rebuilds
def test_refusals_and_rebuilds():
    from mgadmm import _lib
    meta = load_golden("g4_meta.npz")
    y = T_(meta["x_true"][:, :12], torch.float32)
    cl, u, d = tc.tables("knn", 24)

    def unsupported(fn, word):
        with pytest.raises(_lib.MgadmmError) as e:
            fn()
        assert e.value.code == _lib.ERR_UNSUPPORTED and word in str(e.value), str(e.value)

    blk = tc.make_tv_product("knn", 24, 12, tc.info_solve(), path="lds")
    blk.max_ADMM_iter = 3
    unsupported(lambda: blk.solve(y), "LDS-resident path")
    blk.close()

    blk = tc.make_tv_product("knn", 24, 12, tc.info_solve())
    blk.max_ADMM_iter, blk.check_stop = 3, False
    unsupported(lambda: blk.solve(y, sample_params={"rho": [1.0]}), "sample_params")
    unsupported(lambda: blk.solve(y, graph_params={"u_sigma": [2.0]}), "time-varying")
    unsupported(lambda: blk.two_loops(y), "time-varying")
    unsupported(lambda: blk.apply_op_Ln(T_(meta["x_true"], torch.float32)), "time-varying")
    assert blk.CG_iter_x == [] and blk.p_res_list == []      # nothing ran
    h = blk._solvers[(1, torch.float32)][0]
    assert _lib.query(h, _lib.Q_LDS_OK) == 0 and _lib.lib.mgadmm_solver_path(h, 1) == _lib.PATH_STREAM
    # the entry point after a solver exists, with a wrong slice count, and with a value that is not finite
    gph = blk._graphs[1][0]
    nnz_u = int((cl[:, 1:] != -1).sum())
    vals = np.ones((24, nnz_u), dtype=np.float32)
    fp = lambda a: a.ctypes.data_as(_lib._f32p)
    assert _lib.lib.mgadmm_graph_set_time_weights(gph.handle, fp(vals), 24, None, 0) == _lib.ERR_INVALID
    assert b"before a solver is created" in _lib.lib.mgadmm_last_error()
    x1 = blk.solve(y)[0]
    # new varying tables assigned in place rebuild the graph, and the result follows them
    blk.u_ew = torch.from_numpy(np.ascontiguousarray(u[::-1]))
    blk.d_ew = torch.from_numpy(np.ascontiguousarray(d[::-1]))
    x2 = blk.solve(y)[0]
    assert blk._graphs[1][0] is not gph and rel(x2, x1) > 1e-6
    o = tc.TvOracleADMM(cl, u[::-1], d[::-1], tc.info_solve(), mode="knn", t_in=12, T=24)
    assert rel(x2, o.combined_loop(meta["x_true"][:, :12].astype(np.float64), n_iters=3)) < 1e-5
    blk.close()

    from mgadmm.graph import Graph, tables_to_csr
    u_csr, d_csr = tables_to_csr(cl, u[0], 1), tables_to_csr(cl, d[0], 0)
    for kw, word in ((dict(u_val_t=vals[:23]), b"u_val_t: 23 slices"), (dict(d_val_t=np.ones((24, len(d_csr[2])), dtype=np.float32)), b"d_val_t: 24 slices")):
        with pytest.raises(_lib.MgadmmError) as e:
            Graph(30, 24, u_csr, d_csr, **kw)
        assert e.value.code == _lib.ERR_INVALID and word in _lib.lib.mgadmm_last_error()
    bad = vals.copy()
    bad[7, 11] = np.inf
    with pytest.raises(_lib.MgadmmError) as e:
        Graph(30, 24, u_csr, d_csr, u_val_t=bad)
    assert e.value.code == _lib.ERR_INVALID and b"u_val_t[7][11]" in _lib.lib.mgadmm_last_error()
    band = Graph(30, 24, u_csr, None, band_w=np.ones((24, 1), dtype=np.float32), skip=1)
    assert _lib.lib.mgadmm_graph_set_time_weights(band.handle, fp(vals), 24, None, 0) == _lib.ERR_UNSUPPORTED
    band.close()

    # time_varying=True with equal slices: the ordinary one-slice graph, LDS path and all
    blk = tc.make_tv_product("knn", 24, 12, tc.info_solve(), u_ew=np.repeat(u[:1], 24, 0), d_ew=np.repeat(d[:1], 23, 0))
    blk.max_ADMM_iter = 3
    blk.solve(y)
    h = blk._solvers[(1, torch.float32)][0]
    assert not blk._graphs[1][0].time_varying and _lib.query(h, _lib.Q_LDS_OK) == 1 and _lib.lib.mgadmm_solver_path(h, 1) == _lib.PATH_LDS
    blk.close()
