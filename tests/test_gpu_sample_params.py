"""Per-sample ADMM weights on the LDS path (solve(sample_params=...), sweep, mgadmm_solver_set_sample_params): every sample of
a batch solves with its own rho, rho_u, rho_d, mu_u, mu_d1, mu_d2 and equals the solve run alone by an instance carrying those
scalars -- bit for bit against the B = 1 solves of the product (which run k_admm_lds, the batch runs k_admm_lds_pp), within the
project's float32 tolerances against the float64 oracle built with the sample's weights.

Fixture: tables of g4_meta.npz, the 8 inputs y of g5_batched.npz, prediction task, float32, path='lds'; sample b uses the
fixture's six weights times row b of ROWS."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import admm_info_from, load_golden
from helpers import check_windows, make_oracle, make_product, rel

pytestmark = pytest.mark.gpu

F32_X_TOL = 1e-5          # the agreement test_gpu_parity.py demands of float32 solves against the float64 oracle
F32_HIST_RTOL = 1e-3
NAMES = ("rho", "rho_u", "rho_d", "mu_u", "mu_d1", "mu_d2")
ROWS = np.array([
    # rho  rho_u rho_d mu_u mu_d1 mu_d2
    [1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
    [2.0, 1.0, 1.0, 1.0, 1.0, 1.0],
    [0.5, 1.0, 1.0, 1.0, 1.0, 1.0],
    [1.0, 2.0, 0.5, 1.0, 1.0, 1.0],
    [1.0, 0.5, 2.0, 1.0, 1.0, 1.0],
    [1.0, 1.0, 1.0, 2.0, 0.5, 1.0],
    [1.0, 1.0, 1.0, 0.5, 2.0, 2.0],
    [1.5, 0.75, 1.25, 0.25, 4.0, 0.5],
])
CASES = [("knn", "None"), ("knn", "DGLR"), ("line", "None"), ("physical", "DGTV")]
IDS = [f"{m}-{a}" for m, a in CASES]
# the weights an ablation reads ('DGLR' has no zd solve, 'DGTV' no phi: ADMM.py:546-606)
READS = {"None": NAMES, "DGLR": ("rho", "rho_u", "mu_u", "mu_d1"), "DGTV": ("rho_u", "rho_d", "mu_u", "mu_d2")}
FIXED_IT, MAX_IT = 40, 150


def _meta():
    return load_golden("g4_meta.npz")


def _y():
    return torch.from_numpy(load_golden("g5_batched.npz")["y"].astype(np.float32))


def _table(rows=ROWS):
    """sample_params of a batch whose sample b uses the fixture's weights times rows[b] (float64 products)."""
    info = admm_info_from(_meta())
    return {nm: np.array([info[nm] * r[j] for r in rows]) for j, nm in enumerate(NAMES)}


def _row_reads(abl, row):
    return any(row[NAMES.index(nm)] != 1.0 for nm in READS[abl])


def _blk(mode, abl, **kw):
    from mgadmm import _lib
    blk = make_product(_meta(), mode, ablation=abl, path="lds", **kw)
    blk.max_ADMM_iter, blk.check_stop = FIXED_IT, False
    blk.record_cg_coeffs = False              # the chunked schedule (several iterations per launch)
    return blk, _lib


def _carry(blk, table, b):
    """The instance carries sample b's weights as its scalars (the very doubles of the table)."""
    for nm in NAMES:
        setattr(blk, nm, float(table[nm][b]))


def _has(abl):
    return abl in ("None", "DGLR"), abl != "DGLR"


def _snapshot(blk, x, zs, phi, abl):
    has_phi, has_zd = _has(abl)
    cg = [torch.stack([torch.as_tensor(v).reshape(-1) for v in getattr(blk, nm)]).numpy()
          for nm in ("CG_iter_x", "CG_iter_zu") + ("CG_iter_zd",) * has_zd]
    return dict(x=x.clone(), zu=zs[0].clone(), zd=zs[1].clone(), phi=None if phi is None else phi.clone(),
                n=blk.n_iters_per_sample.copy(), mps=blk.metrics_per_sample.copy(), cg=cg, n_iters=len(blk.p_res_list),
                pri=np.array(blk.p_res_list), state={k: v.clone() for k, v in blk.state.items()})


def _solve(blk, y, abl, **kw):
    blk._reset_history()
    x, zs, phi, _ = blk.solve(y, per_sample_history=True, **kw)
    return _snapshot(blk, x, zs, phi, abl)


def _assert_equals_solves_run_alone(one_blk, y, mask, abl, batch, samples, table, what="sample"):
    """Sample b of the batch result against the B = 1 solve of `one_blk` carrying row b's scalars, without a table (so it runs
    k_admm_lds, in whole_batch mode).  Zero tolerance: the two kernels are compiled from one source, the workgroup reads the
    same eight floats (from the table instead of the kernel arguments) and runs the same arithmetic on the same sample."""
    for b in samples:
        _carry(one_blk, table, b)
        one = _solve(one_blk, y[b:b + 1], abl, mask=None if mask is None else mask[b:b + 1])
        nb = one["n_iters"]
        assert int(batch["n"][b]) == nb == int(one["n"][0]), (what, b, batch["n"][b], nb)
        for k in ("x", "zu", "zd", "phi"):
            if one[k] is not None:
                assert torch.equal(batch[k][b], one[k][0]), (what, b, k)
        assert set(batch["state"]) == set(one["state"])
        for k in one["state"]:
            assert torch.equal(batch["state"][k][b], one["state"][k][0]), (what, b, "state", k)
        assert np.array_equal(batch["mps"][:nb, :, b], one["mps"][:, :, 0]), (what, b)
        for cb, c1 in zip(batch["cg"], one["cg"]):
            assert np.array_equal(cb[:nb, b], c1[:, 0]), (what, b)


# ---------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_sweep_batch_equals_the_solves_run_alone_bit_for_bit(i):
    mode, abl = CASES[i]
    blk, lib = _blk(mode, abl)
    h = blk._solver(1, torch.float32, 8)[0]
    assert lib.query(h, lib.Q_LDS_CHUNK) > 1
    y, table = _y(), _table()
    batch = _solve(blk, y, abl, sample_params=table)
    assert batch["n_iters"] == FIXED_IT and (batch["n"] == FIXED_IT).all()
    one_blk, _ = _blk(mode, abl)
    _assert_equals_solves_run_alone(one_blk, y, None, abl, batch, range(8), table)
    # the rows matter to the product too: a sample whose row the ablation reads differs from its solve under row 0
    _carry(one_blk, table, 0)
    for b in range(1, 8):
        x0 = _solve(one_blk, y[b:b + 1], abl)["x"]
        if _row_reads(abl, ROWS[b]):
            assert rel(batch["x"][b:b + 1], x0) > 10 * F32_X_TOL, b
        else:
            assert torch.equal(batch["x"][b:b + 1], x0), b
    blk.close(); one_blk.close()


# ---------------------------------------------------------------------------------------------------------- 2
def _oracle_with_row(mode, abl, table, b):
    o = make_oracle(_meta(), mode, ablation=abl)
    for nm in NAMES:
        setattr(o, nm, float(table[nm][b]))
    return o


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_every_sample_matches_the_oracle_built_with_its_row(i):
    mode, abl = CASES[i]
    blk, _ = _blk(mode, abl)
    y, table = _y(), _table()
    blk._reset_history()
    x = blk.solve(y, per_sample_history=True, sample_params=table)[0]
    y64 = y.double().numpy()
    for b in range(8):
        o = _oracle_with_row(mode, abl, table, b)
        xo = o.combined_loop(y64[b:b + 1], n_iters=FIXED_IT)
        cg = [np.array(getattr(o.hist, nm)) for nm in ("CG_iter_x", "CG_iter_zu") + ("CG_iter_zd",) * _has(abl)[1]]
        assert all((c > 0).all() and c.max() < 100 for c in cg), b               # no solve of the oracle hits the CG limit
        print("sample", b, "rel x", rel(x[b:b + 1], xo), "oracle CG counts", min(c.min() for c in cg), "..", max(c.max() for c in cg))
        check_windows(f"{mode}-{abl} sample {b}", blk, x, [b], o, xo, xtol=F32_X_TOL, htol=F32_HIST_RTOL, slack=1, abl=abl)
        # the fixture discriminates: the oracle's solution under row b is not its solution under row 0
        if b > 0:
            o0 = _oracle_with_row(mode, abl, table, 0)
            x0 = o0.combined_loop(y64[b:b + 1], n_iters=FIXED_IT)
            if _row_reads(abl, ROWS[b]):
                assert rel(xo, x0) > 10 * F32_X_TOL, (b, rel(xo, x0))
            else:
                assert np.array_equal(xo, x0), b
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_a_table_of_equal_rows_is_the_ordinary_solve(i):
    mode, abl = CASES[i]
    blk, lib = _blk(mode, abl)
    y = _y()
    plain = _solve(blk, y, abl)
    h = blk._solvers[(1, torch.float32)][0]
    inst_plain = lib.lds_instance(h)
    same = _solve(blk, y, abl, sample_params=_table(np.repeat(ROWS[:1], 8, 0)))
    assert lib.lds_instance(h) == inst_plain and inst_plain is not None          # the same template arguments ran
    for k in ("x", "zu", "zd", "phi"):
        if plain[k] is not None:
            assert torch.equal(same[k], plain[k]), k
    for k in plain["state"]:
        assert torch.equal(same["state"][k], plain["state"][k]), k
    assert np.array_equal(same["mps"], plain["mps"]) and np.array_equal(same["pri"], plain["pri"])
    for a, b in zip(same["cg"], plain["cg"]):
        assert np.array_equal(a, b)
    # a table that names one weight only: the other five follow the scalars
    part = _solve(blk, y, abl, sample_params={"mu_u": _table()["mu_u"][:1].repeat(8)})
    assert torch.equal(part["x"], plain["x"])
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 4
@functools.lru_cache(maxsize=None)
def _oracle_stops(i):
    """ADMM_tol = median over the samples of the oracle's largest residual at iteration 61 (every sample alone with its row,
    no stop test), and the oracle's stop iteration of every sample at that tolerance."""
    mode, abl = CASES[i]
    y64, table = _y().double().numpy(), _table()
    worst = []
    for b in range(8):
        o = _oracle_with_row(mode, abl, table, b)
        o.ADMM_tol = 0.0
        o.combined_loop(y64[b:b + 1], n_iters=62)
        worst.append(max(max(o.hist.p_res_list[61]), max(o.hist.d_res_list[61])))
    tol = float(np.median(worst))
    stops = []
    for b in range(8):
        o = _oracle_with_row(mode, abl, table, b)
        o.ADMM_tol, o.max_ADMM_iter = tol, MAX_IT
        o.combined_loop(y64[b:b + 1])
        stops.append(len(o.hist.p_res_list))
    return tol, np.array(stops)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_with_per_sample_stopping_every_cell_ends_on_its_own_residuals(i):
    """|n_b - n_b(oracle)| <= 1: the oracle's deciding residual falls by a factor >= 1.0101 per iteration around the stop, ten
    times the 1e-3 agreement demanded of float32 history entries, so the float32 crossing moves by one iteration at most."""
    mode, abl = CASES[i]
    tol, n_orc = _oracle_stops(i)
    print("ADMM_tol", tol, "oracle stops", n_orc.tolist())
    assert n_orc.max() - n_orc.min() >= 20 and n_orc.max() < MAX_IT, n_orc        # the fixture discriminates
    blk, _ = _blk(mode, abl, admm_convergence="per_sample")
    blk.max_ADMM_iter, blk.ADMM_tol, blk.check_stop = MAX_IT, tol, True
    y, table = _y(), _table()
    batch = _solve(blk, y, abl, sample_params=table)
    print("n_b", batch["n"].tolist())
    assert batch["n"].dtype == np.int32 and batch["n_iters"] == batch["n"].max()
    assert np.abs(batch["n"] - n_orc).max() <= 1, (batch["n"], n_orc)
    assert batch["n"].max() - batch["n"].min() >= 20
    one_blk, _ = _blk(mode, abl)
    one_blk.max_ADMM_iter, one_blk.ADMM_tol, one_blk.check_stop = MAX_IT, tol, True
    _assert_equals_solves_run_alone(one_blk, y, None, abl, batch, range(8), table)
    blk.close(); one_blk.close()


# ---------------------------------------------------------------------------------------------------------- 5
def test_interpolation_with_a_float32_mask():
    """g5_batched.npz holds prediction inputs only: its solved x serves as the full series, y = x * mask (as in
    test_gpu_admm_per_sample.py)."""
    meta = _meta()
    xs = load_golden("g5_batched.npz")["x"].astype(np.float64)
    mask64 = np.broadcast_to(meta["mask"].astype(np.float64), xs.shape).copy()
    y, mask = torch.from_numpy((xs * mask64).astype(np.float32)), torch.from_numpy(mask64.astype(np.float32))
    blk, _ = _blk("knn", "None")
    table = _table()
    batch = _solve(blk, y, "None", mask=mask, sample_params=table)
    one_blk, _ = _blk("knn", "None")
    _assert_equals_solves_run_alone(one_blk, y, mask, "None", batch, range(8), table)
    blk.close(); one_blk.close()


# ---------------------------------------------------------------------------------------------------------- 6
def test_more_samples_than_compute_units():
    """B = 1024 = 128 sets x 8 windows (window index fastest): set j is row j mod 8 scaled by 1 + j / 512 in mu_u and rho.
    Per-sample stopping: several rounds of workgroups per CU, cells stop in different launches."""
    mode, abl = CASES[0]
    tol, _ = _oracle_stops(0)
    P, W = 128, 8
    rows = np.repeat(np.stack([ROWS[j % 8] * np.where(np.isin(NAMES, ("mu_u", "rho")), 1 + j / 512, 1.0) for j in range(P)]), W, 0)
    table = _table(rows)
    y = _y().repeat(P, 1, 1, 1)
    blk, lib = _blk(mode, abl, admm_convergence="per_sample")
    blk.max_ADMM_iter, blk.ADMM_tol, blk.check_stop = MAX_IT, tol, True
    batch = _solve(blk, y, abl, sample_params=table)
    n = batch["n"]
    print("B = 1024: n_b min / median / max", n.min(), int(np.median(n)), n.max())
    assert batch["n_iters"] == n.max()
    chunk = lib.query(blk._solvers[(1, torch.float32)][0], lib.Q_LDS_CHUNK)
    assert len({(int(v) - 1) // chunk for v in n}) >= 2, "every cell stopped in the same launch"
    picks = [(j * 67 + 5) % (P * W) for j in range(16)]
    assert len(set(picks)) == 16 and len({(p // W) % 8 for p in picks}) >= 4 and len({p % W for p in picks}) == 8
    one_blk, _ = _blk(mode, abl)
    one_blk.max_ADMM_iter, one_blk.ADMM_tol, one_blk.check_stop = MAX_IT, tol, True
    _assert_equals_solves_run_alone(one_blk, y, None, abl, batch, picks, table)
    blk.close(); one_blk.close()


# ---------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_resume_with_the_same_table(i):
    mode, abl = CASES[i]
    blk, _ = _blk(mode, abl)
    y, table = _y(), _table()
    full = _solve(blk, y, abl, sample_params=table)
    blk.max_ADMM_iter = 15
    first = _solve(blk, y, abl, sample_params=table)
    blk.max_ADMM_iter = FIXED_IT - 15
    second = _solve(blk, y, abl, sample_params=table, warm_start=first["state"])
    assert second["n_iters"] == FIXED_IT - 15
    for k in ("x", "zu", "zd", "phi"):
        if full[k] is not None:
            assert torch.equal(second[k], full[k]), k
    for k in full["state"]:
        assert torch.equal(second["state"][k], full["state"][k]), k
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_recording_cg_coefficients_takes_the_synchronous_schedule_with_the_same_result(i):
    mode, abl = CASES[i]
    has_phi, has_zd = _has(abl)
    blk, _ = _blk(mode, abl)
    y, table = _y(), _table()
    full = _solve(blk, y, abl, sample_params=table)
    blk.record_cg_coeffs = True
    s = _solve(blk, y, abl, sample_params=table)
    assert s["n_iters"] == full["n_iters"] == FIXED_IT
    for k in ("x", "zu", "zd", "phi"):
        if full[k] is not None:
            assert torch.equal(s[k], full[k]), k
    for k in full["state"]:
        assert torch.equal(s["state"][k], full["state"][k]), k
    assert np.array_equal(s["mps"], full["mps"]) and np.array_equal(s["pri"], full["pri"])
    for a, b in zip(s["cg"], full["cg"]):
        assert np.array_equal(a, b)
    for w, (al, be) in enumerate(((blk.alpha_x, blk.beta_x), (blk.alpha_zu, blk.beta_zu)) + (((blk.alpha_zd, blk.beta_zd),) * has_zd)):
        al, be = torch.stack(al).numpy(), torch.stack(be).numpy()          # (iters, max_CG_iter, B)
        assert al.shape[0] == FIXED_IT
        for b in range(8):
            for it in range(FIXED_IT):
                k = int(s["cg"][w][it, b])
                assert k > 0 and np.isfinite(al[it, :k, b]).all() and np.isfinite(be[it, :k, b]).all(), (w, b, it)
                assert np.isnan(al[it, k:, b]).all(), (w, b, it)
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 9
def test_sweep_returns_the_grid_of_solves():
    mode, abl = CASES[0]
    blk, _ = _blk(mode, abl)
    y = _y()
    grid = {"mu_u": [0.5, 1, 2], "mu_d1": [1, 2]}
    x, n, sets = blk.sweep(y, grid)
    assert tuple(x.shape) == (6, 8, 24, 30, 1) and n.shape == (6, 8) and (n == FIXED_IT).all()
    assert sets == [dict(mu_u=a, mu_d1=b) for a in (0.5, 1, 2) for b in (1, 2)]
    one_blk, _ = _blk(mode, abl)
    for p, w in [(0, 0), (1, 3), (2, 7), (3, 4), (4, 1), (5, 6)]:
        one_blk.mu_u, one_blk.mu_d1 = float(sets[p]["mu_u"]), float(sets[p]["mu_d1"])
        assert torch.equal(x[p, w], one_blk.solve(y[w:w + 1])[0][0]), (p, w)
    x2, n2, sets2 = blk.sweep(y, grid, chunk=16)                 # three solves of 16 samples
    assert torch.equal(x2, x) and np.array_equal(n2, n) and sets2 == sets
    blk.close(); one_blk.close()


# ---------------------------------------------------------------------------------------------------------- 10
def test_cleared_means_cleared():
    mode, abl = CASES[0]
    blk, lib = _blk(mode, abl)
    y = _y()
    _solve(blk, y, abl, sample_params=_table())
    after = _solve(blk, y, abl)
    fresh_blk, _ = _blk(mode, abl)
    fresh = _solve(fresh_blk, y, abl)
    for k in fresh["state"]:
        assert torch.equal(after["state"][k], fresh["state"][k]), k
    assert np.array_equal(after["mps"], fresh["mps"])
    # also after a call that failed in the library: the table does not outlive it
    blk.check_stop = True                                       # whole_batch stop test with a table: refused
    with pytest.raises(lib.MgadmmError):
        blk.solve(y, sample_params=_table())
    blk.check_stop = False
    assert torch.equal(_solve(blk, y, abl)["x"], fresh["x"])
    blk.close(); fresh_blk.close()


# ---------------------------------------------------------------------------------------------------------- 11
def _expect_unsupported(blk, y, lib, reason, table=None):
    blk._reset_history()
    with pytest.raises(lib.MgadmmError) as e:
        blk.solve(y, sample_params=_table() if table is None else table)
    assert e.value.code == lib.ERR_UNSUPPORTED, e.value
    assert "sample_params" in str(e.value) and reason in str(e.value), e.value
    assert blk.p_res_list == []                                  # nothing ran
    x = blk.solve(y)[0]                                          # the same instance still solves normally
    assert torch.isfinite(x).all() and len(blk.p_res_list) > 0


def test_refused_on_the_streaming_path():
    blk, lib = _blk("knn", "None")
    blk.path, blk.max_ADMM_iter = "stream", 3
    _expect_unsupported(blk, _y(), lib, "MGADMM_PATH_STREAM")
    blk.close()


def test_refused_in_float64():
    from mgadmm import _lib as lib
    blk = make_product(_meta(), "knn", compute_dtype=torch.float64)
    blk.max_ADMM_iter, blk.check_stop = 3, False
    _expect_unsupported(blk, _y().double(), lib, "float64")
    blk.close()


def test_refused_with_batch_max_cg_convergence():
    from mgadmm import _lib as lib
    blk = make_product(_meta(), "knn", cg_convergence="batch_max")
    blk.max_ADMM_iter, blk.check_stop = 3, False
    _expect_unsupported(blk, _y(), lib, "batch_max")
    blk.close()


def test_refused_for_a_graph_beyond_the_lds_path():
    from mgadmm import _lib as lib
    from mgadmm.ADMM import ADMM_algorithm
    rng = np.random.default_rng(5)
    N, k = 600, 4
    pts = rng.random((N, 2))
    d = np.linalg.norm(pts[:, None] - pts[None], axis=2)
    cl = np.argsort(d, axis=1)[:, :k + 1]
    cl[:, 0] = np.arange(N)
    dl = np.take_along_axis(d, cl, 1).astype(np.float32)
    r = (N / 24) ** 0.5
    info = dict(rho=2 * r, rho_u=3 * r, rho_d=2 * r, mu_u=1, mu_d1=2, mu_d2=1)
    blk = ADMM_algorithm({"n_nodes": N}, info, use_kNN=True, k=k, u_sigma=1.0, d_sigma=1.0,
                         tables=(torch.from_numpy(cl), torch.from_numpy(dl)))
    blk.max_ADMM_iter, blk.check_stop = 3, False
    y = torch.from_numpy((1 + rng.random((2, 12, N, 1))).astype(np.float32))
    _expect_unsupported(blk, y, lib, "cannot hold this graph", table={"mu_u": [1.0, 2.0]})
    blk.close()


def test_refused_with_the_whole_batch_stop_test():
    blk, lib = _blk("knn", "None")
    blk.check_stop, blk.ADMM_tol, blk.max_ADMM_iter = True, 1e-6, 5
    assert blk.admm_convergence == "whole_batch"
    _expect_unsupported(blk, _y(), lib, "whole_batch")
    blk.close()


def test_invalid_tables_straight_through_the_c_abi():
    blk, lib = _blk("knn", "None")
    y = _y()
    blk.max_ADMM_iter = 3
    blk.solve(y)                                                 # the solver exists, max_batch = 8
    h = blk._solvers[(1, torch.float32)][0]
    setp = lib.lib.mgadmm_solver_set_sample_params
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    err = lambda: lib.lib.mgadmm_last_error().decode()

    ones9 = np.ones(9)
    sp = lib.SampleParams(rho=dp(ones9))
    assert setp(h, C.byref(sp), 9) == lib.ERR_INVALID and "max_batch" in err()           # B > max_batch
    rho = np.ones(8); rho[3] = 0.0
    assert setp(h, C.byref(lib.SampleParams(rho=dp(rho))), 8) == lib.ERR_INVALID and "rho[3]" in err()
    mu = np.ones(8); mu[5] = np.nan
    assert setp(h, C.byref(lib.SampleParams(mu_u=dp(mu))), 8) == lib.ERR_INVALID and "mu_u[5]" in err()
    neg = np.ones(8); neg[7] = -1.0
    assert setp(h, C.byref(lib.SampleParams(mu_d2=dp(neg))), 8) == lib.ERR_INVALID and "mu_d2[7]" in err()
    # a refused table leaves none behind
    blk._reset_history()
    x_plain = blk.solve(y)[0]
    # table B != solve B
    four = np.ones(4) * float(blk.mu_u)
    assert setp(h, C.byref(lib.SampleParams(mu_u=dp(four))), 4) == lib.OK
    blk._reset_history()
    with pytest.raises(lib.MgadmmError) as e:
        blk.solve(y)
    assert e.value.code == lib.ERR_INVALID and "4 samples" in str(e.value) and blk.p_res_list == []
    assert setp(h, None, 0) == lib.OK
    assert torch.equal(blk.solve(y)[0], x_plain)
    blk.close()
