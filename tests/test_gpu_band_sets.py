"""Per-sample temporal band weights (solve(band_params=...), solve(band_sets=...), sweep(skips=...),
mgadmm_solver_set_sample_bands): sample b of a batch on a line-graph instance of width 6 reads its own band table.

  * LDS-resident path (float32, kernels k_admm_lds_pp): every sample equals, bit for bit, the B = 1 solve of an instance built
    with skip_connection = s at its NATIVE width (the decaying set: a width-6 instance whose d_ew is overwritten), which runs
    k_admm_lds -- a narrower interval is the wide table with zero hops, and `acc += 0 * v` leaves an accumulator that started
    at +0 bit for bit;
  * streaming path (float32 and float64): the geometry depends on B, so the twin is the whole batch solved on an instance of
    set s; every sample of the table solve whose set is s equals that solve's sample bit for bit;
  * both against the float64 oracle run per sample with the sample's table, at the project's tolerances;
  * every BAND instance of k_admm_lds_pp (the ten band rows of tests/lds_census.py, widths 1 and 3): three samples of one
    window under the graph's own table times 1, 0.5 and 0.25 against B = 1 solves of instances carrying that table, bit for bit.

The problem (tests/band_sets_cases.py) is the smallest on which each kernel can go wrong; every test asserts that two samples
of one window under different sets differ by more than 100 x its tolerance, so a kernel that ignores the table cannot pass."""
import ctypes as C

import numpy as np
import pytest
import torch

import band_sets_cases as bc
import lds_census as lc
from conftest import admm_info_from
from helpers import check_windows
from test_gpu_lds_census import _info, _inputs, _product, env  # noqa: F401
from test_gpu_sample_params import _solve

pytestmark = pytest.mark.gpu

B15 = 15
LDS_IT, STREAM_IT = 6, 3


def _prep(blk, iters, **attrs):
    blk.max_ADMM_iter, blk.check_stop, blk.record_cg_coeffs = iters, False, False      # several iterations per launch
    for k, v in attrs.items():
        setattr(blk, k, v)
    return blk


def _band_kw(B):
    """The band arguments of a batch of B samples.  A solver of max_batch = B takes at most B tables: a batch smaller than the
    five sets passes the sets its samples use, in order of first appearance (B = 3: sets 0, 3, 1)."""
    tabs, sos = bc.tables(), bc.set_of_sample(B)
    if B >= bc.N_SETS:
        return dict(band_sets=tabs, band_of_sample=sos)
    used = list(dict.fromkeys(int(j) for j in sos))
    return dict(band_sets=[tabs[j] for j in used], band_of_sample=np.array([used.index(int(j)) for j in sos], dtype=np.int32))


def _handle(blk, dtype=torch.float32):
    return blk._solvers[(1, dtype)][0]


def _unit(blk):
    from mgadmm import _lib
    return _lib.query(_handle(blk), _lib.Q_LDS_UNIT)


def _path(blk, B, dtype=torch.float32):
    from mgadmm import _lib
    return _lib.lib.mgadmm_solver_path(_handle(blk, dtype), B)


def _assert_sets_discriminate(x, B, tol):
    """Two samples of one window under different sets differ by more than 100 x the test's tolerance."""
    sos, win = bc.set_of_sample(B), bc.window_of_sample(B)
    pairs = [(b, b + 1) for b in range(B - 1) if win[b] == win[b + 1] and sos[b] != sos[b + 1]]
    assert pairs
    worst = min(bc.predicted_difference(x, a, b) for a, b in pairs)
    print(f"smallest difference between two sets on one window: {worst:.3e} (tolerance {tol:g})")
    assert worst > 100 * tol, (worst, tol)


def _assert_sample_equals(batch, b, one, b1, what):
    nb = int(one["n"][b1])
    assert int(batch["n"][b]) == nb, (what, b, batch["n"][b], nb)
    for k in ("x", "zu", "zd", "phi"):
        if one[k] is not None:
            assert torch.equal(batch[k][b], one[k][b1]), (what, b, k)
    assert set(batch["state"]) == set(one["state"])
    for k in one["state"]:
        assert torch.equal(batch["state"][k][b], one["state"][k][b1]), (what, b, "state", k)
    assert np.array_equal(batch["mps"][:nb, :, b], one["mps"][:nb, :, b1]), (what, b, "metrics_per_sample")
    for cb, c1 in zip(batch["cg"], one["cg"]):
        assert np.array_equal(cb[:nb, b], c1[:nb, b1]), (what, b, "CG counts")


def _assert_equals_b1_twins(abl, batch, y, mask, prepare, table=None, what="sample"):
    """Every sample of the B = 15 batch against the B = 1 solve of the instance built with its set at the native width."""
    from mgadmm import _lib
    sos = bc.set_of_sample(B15)
    twins = {}
    for b in range(B15):
        j = int(sos[b])
        if j not in twins:
            twins[j] = prepare(bc.twin(abl, j, path="lds"))
        t = twins[j]
        if table is not None:
            for nm, col in table.items():
                setattr(t, nm, float(col[b]))
        one = _solve(t, y[b:b + 1], abl, mask=None if mask is None else mask[b:b + 1])
        assert _lib.query(_handle(t), _lib.Q_LDS_UNIT) == 0, (what, b)           # the twin ran k_admm_lds
        _assert_sample_equals(batch, b, one, 0, what)
    for t in twins.values():
        t.close()


# ---------------------------------------------------------------------------------------------------------- 1
LDS_CASES = [("None", "pred"), ("DGLR", "pred"), ("DGTV", "pred"), ("None", "mask")]


@pytest.mark.parametrize("abl, task", LDS_CASES, ids=[f"{a}-{t}" for a, t in LDS_CASES])
def test_lds_batch_of_15_equals_the_native_width_solves_run_alone(abl, task):
    from mgadmm import _lib
    y, mask = bc.inputs(B15, task)
    blk = _prep(bc.instance(abl, path="lds"), LDS_IT)
    batch = _solve(blk, y, abl, mask=mask, **_band_kw(B15))
    assert _path(blk, B15) == _lib.PATH_LDS and _unit(blk) == 2
    assert batch["n_iters"] == LDS_IT and (batch["n"] == LDS_IT).all()
    _assert_sets_discriminate(batch["x"], B15, bc.F32_TOL["xtol"])
    assert bc.min_set_difference(abl, LDS_IT, task) > 100 * bc.F32_TOL["xtol"]
    _assert_equals_b1_twins(abl, batch, y, mask, lambda t: _prep(t, LDS_IT))
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 2
def test_lds_with_sample_params_and_per_sample_stopping(env):
    """Band table + sample_params (three mu_d1 values) + admm_convergence='per_sample'.  ADMM_tol by lc.pick_admm_tol on the
    ORACLE's deciding residuals of the fifteen samples (no residual within 1 % of it): the samples stop at iterations 3, 4
    and 5, in different launches of 2."""
    from mgadmm import _lib
    abl, K, chunk = "DGLR", LDS_IT, 2
    env.setenv("MGADMM_LDS_CHUNK", str(chunk))
    y, _ = bc.inputs(B15)
    sos, tabs, info0 = bc.set_of_sample(B15), bc.tables(), admm_info_from(bc.meta())
    table = {"mu_d1": np.array([info0["mu_d1"] * (0.5, 1.0, 2.0)[b % 3] for b in range(B15)])}
    res = []
    for b in range(B15):
        o = bc.oracle(abl, tabs[sos[b]], dict(info0, mu_d1=float(table["mu_d1"][b])))
        o.combined_loop(y[b:b + 1].double().numpy(), n_iters=K)
        res.append(np.maximum(np.array(o.hist.p_res_list).max(1), np.array(o.hist.d_res_list).max(1)))
    tol, n_first = lc.pick_admm_tol(np.stack(res), K, chunk=chunk)
    print("\nADMM_tol", tol, "first crossings", n_first)
    blk = _prep(bc.instance(abl, path="lds", admm_convergence="per_sample"), K, ADMM_tol=tol, check_stop=True)
    batch = _solve(blk, y, abl, sample_params=table, **_band_kw(B15))
    assert _unit(blk) == 2 and _lib.query(_handle(blk), _lib.Q_LDS_CHUNK) == chunk
    assert batch["n"].tolist() == n_first and batch["n_iters"] == max(n_first) and len(set(n_first)) >= 2
    _assert_sets_discriminate(batch["x"], B15, bc.F32_TOL["xtol"])
    _assert_equals_b1_twins(abl, batch, y, None, lambda t: _prep(t, K, ADMM_tol=tol, check_stop=True), table=table)
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 3
STREAM_CASES = [(torch.float32, 3, "None"), (torch.float32, 100, "DGLR"), (torch.float32, 260, "DGTV"), (torch.float64, 130, "None")]


@pytest.mark.parametrize("dtype, B, abl", STREAM_CASES, ids=[f"{str(d).split('.')[1]}-B{B}-{a}" for d, B, a in STREAM_CASES])
def test_streaming_batch_equals_the_whole_batch_twins(dtype, B, abl):
    """VEC 1 (B = 3), VEC 2 with Bp = 128 (B = 100), VEC 4 with two column chunks and 252 padded columns (B = 260), float64
    VEC 2 with two chunks (B = 130)."""
    from mgadmm import _lib
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    y, _ = bc.inputs(B, "pred", np_dtype)
    sos = bc.set_of_sample(B)
    blk = _prep(bc.instance(abl, path="stream", compute_dtype=dtype), STREAM_IT)
    batch = _solve(blk, y, abl, **_band_kw(B))
    assert _path(blk, B, dtype) == _lib.PATH_STREAM
    assert batch["n_iters"] == STREAM_IT and batch["x"].dtype == dtype
    _assert_sets_discriminate(batch["x"], B, (bc.F32_TOL if dtype == torch.float32 else bc.F64_TOL)["xtol"])
    for j in range(bc.N_SETS):
        t = _prep(bc.twin(abl, j, path="stream", compute_dtype=dtype), STREAM_IT)
        whole = _solve(t, y, abl)
        for b in np.nonzero(sos == j)[0]:
            _assert_sample_equals(batch, int(b), whole, int(b), f"set {j}")
        t.close()
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 4
ORACLE_CASES = [("lds", torch.float32, "None"), ("stream", torch.float32, "DGLR"), ("stream", torch.float64, "DGTV")]


@pytest.mark.parametrize("path, dtype, abl", ORACLE_CASES, ids=[f"{p}-{str(d).split('.')[1]}-{a}" for p, d, a in ORACLE_CASES])
def test_batch_of_15_against_the_oracle_with_each_samples_table(path, dtype, abl):
    f32 = dtype == torch.float32
    tol = bc.F32_TOL if f32 else bc.F64_TOL
    y, _ = bc.inputs(B15, "pred", np.float32 if f32 else np.float64)
    sos, tabs = bc.set_of_sample(B15), bc.tables()
    blk = _prep(bc.instance(abl, path=path, compute_dtype=dtype), LDS_IT)
    x = blk.solve(y, per_sample_history=True, **_band_kw(B15))[0]
    _assert_sets_discriminate(x, B15, tol["xtol"])
    assert bc.min_set_difference(abl, LDS_IT) > 100 * bc.F32_TOL["xtol"]
    for b in range(B15):
        o = bc.oracle(abl, tabs[sos[b]])
        xo = o.combined_loop(y[b:b + 1].double().numpy(), n_iters=LDS_IT)
        check_windows(f"{path} sample {b} set {sos[b]}", blk, x, [b], o, xo, abl=abl, **tol)
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 5
def _setb(h, tables, sos, B):
    from mgadmm import _lib
    tables = np.ascontiguousarray(tables, dtype=np.float32)
    sos = np.ascontiguousarray(sos, dtype=np.int32)
    rc = _lib.lib.mgadmm_solver_set_sample_bands(h, len(tables), tables.ctypes.data_as(C.POINTER(C.c_float)),
                                                 sos.ctypes.data_as(C.POINTER(C.c_int32)), B)
    return rc, _lib.lib.mgadmm_last_error().decode()


def _clear(h):
    from mgadmm import _lib
    return _lib.lib.mgadmm_solver_set_sample_bands(h, 0, None, None, 0)


def test_refusals_by_code_and_message():
    from mgadmm import _lib
    import graph_sets_cases as gc
    B = 5
    y, _ = bc.inputs(B)
    tabs, sos = np.stack(bc.tables()), bc.set_of_sample(B)
    # a spatial temporal graph has no band table
    knn = gc.instance("knn", "None", *gc.pairs()[1], path="lds")
    knn.max_ADMM_iter, knn.check_stop = 2, False
    x_knn = knn.solve(y)[0]
    rc, msg = _setb(_handle(knn), tabs, sos, B)
    assert rc == _lib.ERR_UNSUPPORTED and msg.startswith("set_sample_bands: the solver's graph is not MGADMM_TEMPORAL_BAND"), msg
    with pytest.raises(ValueError, match="no line graph"):
        knn.solve(y, **_band_kw(B))
    assert torch.equal(knn.solve(y)[0], x_knn)
    knn.close()

    blk = _prep(bc.instance("None", path="lds"), 2)
    x_plain = blk.solve(y)[0]                                   # the solver exists, max_batch = 5
    h = _handle(blk)
    # index out of range, non-finite entry, B and n_sets outside [1, max_batch]
    bad = sos.copy(); bad[3] = 5
    rc, msg = _setb(h, tabs, bad, B)
    assert rc == _lib.ERR_INVALID and msg == "set_sample_bands: set_of_sample[3] = 5 outside [0, n_sets=5)", msg
    badw = tabs.copy(); badw[4, 7, 2] = np.inf
    rc, msg = _setb(h, badw, sos, B)
    assert rc == _lib.ERR_INVALID and msg == "set_sample_bands: band_w[4][7][2] is not finite", msg
    badw = tabs.copy(); badw[1, 2, 2:] = np.nan; badw[:, 0, :] = np.nan       # entries no operator reads are ignored
    assert _setb(h, badw, sos, B)[0] == _lib.OK and _clear(h) == _lib.OK
    rc, msg = _setb(h, tabs, np.zeros(6, np.int32), 6)
    assert rc == _lib.ERR_INVALID and msg == "set_sample_bands: batch 6 outside [1, max_batch=5]", msg
    rc, msg = _setb(h, np.concatenate([tabs, tabs[:1]]), sos, B)
    assert rc == _lib.ERR_INVALID and msg == "set_sample_bands: n_sets 6 outside [1, max_batch=5]", msg
    assert torch.equal(blk.solve(y)[0], x_plain)                 # none of the refused calls left a table behind
    # B mismatch: a table of 4 samples, a solve of 5
    assert _setb(h, tabs, sos[:4], 4)[0] == _lib.OK
    blk._reset_history()
    with pytest.raises(_lib.MgadmmError) as e:
        blk.solve(y)
    assert e.value.code == _lib.ERR_INVALID and "the sample_bands table holds 4 samples, the solve has B = 5" in str(e.value)
    assert blk.p_res_list == [] and _clear(h) == _lib.OK
    # the whole-batch stop test
    blk.check_stop, blk.ADMM_tol = True, 1e-6
    blk._reset_history()
    with pytest.raises(_lib.MgadmmError) as e:
        blk.solve(y, **_band_kw(B))
    assert e.value.code == _lib.ERR_UNSUPPORTED and "sample_bands with check_stop need admm_convergence per_sample" in str(e.value)
    assert blk.p_res_list == []
    blk.check_stop = False
    assert torch.equal(blk.solve(y)[0], x_plain)
    # with sample_params also set on the streaming path, the sample_params refusal answers first
    blk.path = "stream"
    blk._reset_history()
    with pytest.raises(_lib.MgadmmError) as e:
        blk.solve(y, sample_params={"rho": [1.0] * B}, **_band_kw(B))
    assert e.value.code == _lib.ERR_UNSUPPORTED and "sample_params" in str(e.value) and "sample_bands" not in str(e.value), e.value
    assert blk.p_res_list == []
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("path", ["lds", "stream"])
def test_lifetime_of_the_table(path):
    from mgadmm import _lib
    abl, B = "None", 5
    y, _ = bc.inputs(B)
    tabs, sos = np.stack(bc.tables()), bc.set_of_sample(B)
    fresh = _prep(bc.instance(abl, path=path), STREAM_IT)
    x_fresh = fresh.solve(y)[0]
    fresh.close()
    blk = _prep(bc.instance(abl, path=path), STREAM_IT)
    x_band = blk.solve(y, **_band_kw(B))[0]
    _assert_sets_discriminate(x_band, B, bc.F32_TOL["xtol"])
    assert not torch.equal(x_band, x_fresh)
    assert torch.equal(blk.solve(y)[0], x_fresh)                 # the table does not outlive solve(band_sets=...)
    # ... also when the solve inside the scope was refused
    blk.check_stop = True
    with pytest.raises(_lib.MgadmmError):
        blk.solve(y, **_band_kw(B))
    blk.check_stop = False
    assert torch.equal(blk.solve(y)[0], x_fresh)
    # through the C ABI: set_params keeps the table, clearing gives the plain solve
    h = _handle(blk)
    assert _setb(h, tabs, sos, B)[0] == _lib.OK
    assert torch.equal(blk.solve(y)[0], x_band)                  # (every solve() calls mgadmm_solver_set_params first)
    blk.max_CG_iter += 1                                         # ... also with other parameters
    assert torch.equal(blk.solve(y)[0], x_band)
    assert _clear(h) == _lib.OK
    assert torch.equal(blk.solve(y)[0], x_fresh)
    # the operator methods keep reading the graph's own table while one is set
    ldr = blk.apply_op_Ldr(x_fresh)
    assert _setb(h, tabs, sos, B)[0] == _lib.OK
    assert torch.equal(blk.apply_op_Ldr(x_fresh), ldr)
    assert _clear(h) == _lib.OK
    blk.close()


def test_band_params_equals_the_low_level_form():
    abl = "DGLR"
    y, _ = bc.inputs(B15)
    skips = [bc.INTERVALS[b % 4] for b in range(B15)]
    blk = _prep(bc.instance(abl, path="lds"), STREAM_IT)
    a = _solve(blk, y, abl, band_params={"skip": skips})
    sets = [bc.uniform_table(s) for s in bc.INTERVALS]
    b = _solve(blk, y, abl, band_sets=sets, band_of_sample=[i % 4 for i in range(B15)])
    assert _unit(blk) == 2 and torch.equal(a["x"], b["x"]) and np.array_equal(a["mps"], b["mps"])
    c = blk.combined_loop(y, print_info=False, band_params={"skip": skips})
    assert torch.equal(c, a["x"])
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 7
def test_sweep_over_skip_connection_intervals():
    abl = "None"
    y, _ = bc.inputs(B15)
    y = y[::5]                                                   # the three windows
    blk = _prep(bc.instance(abl, path="lds"), STREAM_IT)
    x, n, sets = blk.sweep(y, {"mu_d1": [1, 2]}, skips=[1, 3, 6])
    T, _, N = bc.dims()
    assert tuple(x.shape) == (6, 3, T, N, 1) and (n == STREAM_IT).all()
    assert sets == [dict(mu_d1=m, skip=s) for m in (1, 2) for s in (1, 3, 6)]          # itertools.product order, 'skip' last
    assert _unit(blk) == 2
    for w in range(3):
        for p0, p1 in ((0, 1), (1, 2), (3, 5)):
            d = float((x[p0, w, 12:] - x[p1, w, 12:]).norm() / x[p1, w, 12:].norm())
            assert d > 100 * bc.F32_TOL["xtol"], (w, p0, p1, d)
    for p, s in enumerate(sets):
        one = _prep(bc.instance(abl, s["skip"], path="lds"), STREAM_IT, mu_d1=float(s["mu_d1"]))
        for w in range(3):
            assert torch.equal(x[p, w], one.solve(y[w:w + 1])[0][0]), (p, w)
        one.close()
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 8
BAND_ROWS = [r for r in lc.CENSUS if r["expect"].split(", ")[1] == "true"]      # the ten BAND instances
ROW_FACTORS = (1.0, 0.5, 0.25)          # the graph's own table times a power of two: exact in float32 at width 1 and width 3
ROW_SET_OF_SAMPLE = [2, 0, 1]
ROW_IT = 3


@pytest.mark.parametrize("r", BAND_ROWS, ids=lc.row_id)
def test_every_band_instance_reads_the_table_of_its_sample(r, env):
    """Every BAND instance of k_admm_lds_pp (the census row's problem, with the zd solve on so the trip reads the temporal rows
    twice): ONE window three times in a batch, sample b under the graph's own band table times ROW_FACTORS[ROW_SET_OF_SAMPLE[b]],
    three iterations.  The launch reports unit 2 and the row's instance; every sample equals, bit for bit, the B = 1 solve of
    an instance whose d_ew is overwritten with its set (k_admm_lds, unit 0); the three solutions, which differ by nothing
    but the table, lie more than 100 x the float32 tolerance apart."""
    from mgadmm import _lib
    assert len(BAND_ROWS) == 10
    for k, v in r["env"].items():
        env.setenv(k, v)
    B, abl = len(ROW_SET_OF_SAMPLE), "None" if r["abl"] == "DGLR" else r["abl"]          # 'DGLR' has no zd solve
    r = dict(r, abl=abl, B=1)
    info = _info(r["N"], r["T"])
    y1, m1 = _inputs(r)
    y = torch.from_numpy(y1).repeat(B, 1, 1, 1)
    mask = None if m1 is None else torch.from_numpy(m1).repeat(B, 1, 1, 1)
    tag = f"{r['expect']} N={r['N']} T={r['T']} {r['kind']} {abl} {r['task']}"

    blk = _prep(_product(r, info, path="lds"), ROW_IT)
    own = blk.d_ew[:, :, 0].numpy().copy()                                               # (T, skip) float32
    sets = [own * np.float32(f) for f in ROW_FACTORS]
    batch = _solve(blk, y, abl, mask=mask, band_sets=sets, band_of_sample=np.array(ROW_SET_OF_SAMPLE, dtype=np.int32))
    assert _path(blk, B) == _lib.PATH_LDS and _unit(blk) == 2, tag
    assert _lib.lds_instance(_handle(blk)) == r["expect"], (tag, _lib.lds_instance(_handle(blk)))
    assert batch["n_iters"] == ROW_IT and (batch["n"] == ROW_IT).all(), tag
    blk.close()

    for b, j in enumerate(ROW_SET_OF_SAMPLE):
        t = _prep(_product(r, info, path="lds"), ROW_IT)
        t.d_ew = torch.from_numpy(sets[j])[:, :, None].repeat(1, 1, r["N"])
        one = _solve(t, y[b:b + 1], abl, mask=None if mask is None else mask[b:b + 1])
        assert _unit(t) == 0 and _lib.lds_instance(_handle(t)) == r["expect"], (tag, b)
        _assert_sample_equals(batch, b, one, 0, tag)
        t.close()

    x = batch["x"].double()
    apart = [float((x[a] - x[b]).norm() / x[b].norm()) for a, b in ((0, 1), (0, 2), (1, 2))]
    print(f"\n[band rows] {tag}: the three sets apart by {apart}")
    assert min(apart) > 100 * bc.F32_TOL["xtol"], (tag, apart)
