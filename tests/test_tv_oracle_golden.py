"""tests/tv_oracle.py (the float64 restatement over per-slice CSR matrices) pinned against tests/golden/g11_time_varying.npz, the
reference's own output on tables that vary over time (tests/golden/gen_golden_tv.py), at the tolerances tests/test_oracle_golden.py
uses for the time-invariant restatement."""
import numpy as np
import pytest

import tv_cases as tc
from test_oracle_golden import RTOL64, rel

MODES = ("knn", "physical")


def test_fixture_tables_vary_in_every_entry():
    g = tc.g11()
    for mode in MODES:
        u, d = g[mode + "_u_ew"], g[mode + "_d_ew"]
        assert u.shape[0] == int(g["T"]) and d.shape[0] == int(g["T"]) - 1
        assert (u[1:] != u[:-1])[u[1:] != 0].all() and (d[1:] != d[:-1])[d[1:] != 0].all()


@pytest.mark.parametrize("mode", MODES)
def test_dense_operators_and_left_hand_sides(mode):
    g = tc.g11()
    o = tc.make_tv_oracle(mode, int(g["T_ops"]), int(g["t_in_ops"]), tc.info_ops())
    G = lambda nm: g[f"ops/{mode}/{nm}"]
    for nm in ("Lu", "Ldr", "Ldr_T", "cLdr"):
        assert rel(o.dense(getattr(o, "apply_op_" + nm)), G(nm)) < 1e-14, nm
    assert rel(o.dense(o.LHS_zu), G("LHS_zu")) < 1e-14
    assert rel(o.dense(o.LHS_zd), G("LHS_zd")) < 1e-14
    assert rel(o.dense(o.LHS_x), G("LHS_x")) < 1e-14
    m = g["ops/mask"]
    assert rel(o.dense(lambda e: o.LHS_x(e, mask=m)), G("LHS_x_mask")) < 1e-14
    # the slices are really read: the restatement on slice 0 alone is another matrix
    from oracle import admm_oracle as orc
    cl, u, d = tc.tables(mode, int(g["T_ops"]))
    o0 = orc.OracleADMM(cl, u[0], d[0], tc.info_ops(), mode=mode, t_in=int(g["t_in_ops"]), T=int(g["T_ops"]))
    for nm in ("Lu", "Ldr", "Ldr_T"):
        assert rel(o0.dense(getattr(o0, "apply_op_" + nm)), G(nm)) > 1e-4, nm


@pytest.mark.parametrize("mode", MODES)
def test_cg(mode):
    g = tc.g11()
    o = tc.make_tv_oracle(mode, int(g["T_ops"]), int(g["t_in_ops"]), tc.info_ops())
    rhs, x0, m = g["cg/rhs"], g["cg/x0"], g["ops/mask"].astype(np.float64)
    for nm, fn, kw in (("x", o.LHS_x, {}), ("xmask", o.LHS_x, {"mask": m}), ("zu", o.LHS_zu, {}), ("zd", o.LHS_zd, {})):
        x, it, al, be = o.CG_solver(fn, rhs, x0, **kw)
        pre = f"cg/{mode}/{nm}_"
        assert int(it[0]) == int(g[pre + "iters"]), nm
        assert rel(x, g[pre + "x"]) < RTOL64
        np.testing.assert_allclose(al[:, 0], g[pre + "alpha"], rtol=2e-7)
        np.testing.assert_allclose(be[:, 0], g[pre + "beta"], rtol=2e-7, atol=1e-12)


@pytest.mark.parametrize("task", ["pred", "mask"])
@pytest.mark.parametrize("mode", MODES)
def test_full_solves(mode, task):
    from test_oracle_golden import case_inputs
    from conftest import load_golden
    g, meta = tc.g11(), load_golden("g4_meta.npz")
    key = f"{mode}-None-{task}-f64-10"
    G = lambda f: g[f"{key}/{f}"]
    o = tc.make_tv_oracle(mode, int(g["T"]), int(g["t_in"]), tc.info_solve())
    y, mask = case_inputs(meta, task, "f64")
    o.max_ADMM_iter = 10
    x = o.combined_loop(y, mask=mask)
    h = o.hist
    assert int(G("n_iters")) == 10 and len(h.p_res_list) == 10
    assert rel(x, G("x")) < 1e-11
    for nm in ("CG_iter_x", "CG_iter_zu", "CG_iter_zd"):
        assert np.array_equal(np.array([int(v[0]) for v in getattr(h, nm)]), G(nm)), nm
    np.testing.assert_allclose(h.DGLR_list, G("DGLR"), rtol=1e-9)
    np.testing.assert_allclose(h.DGTV_list, G("DGTV"), rtol=1e-9)
    np.testing.assert_allclose(h.GLR_list, G("GLR"), rtol=1e-9)
    np.testing.assert_allclose(np.array(h.p_res_list), G("p_res"), rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(np.array(h.d_res_list), G("d_res"), rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(h.x_shift_list, G("x_shift"), rtol=1e-8)
    np.testing.assert_allclose(np.array(h.delta_x_per_step), G("dxps"), rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(h.recover_list, G("recover"), rtol=1e-8, atol=1e-12)
    for nm, tol in (("zu", 1e-11), ("zd", 1e-11), ("phi", 1e-10)):
        assert rel(o.state[nm], G(nm)) < tol, nm
