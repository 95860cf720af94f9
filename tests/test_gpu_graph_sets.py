"""Per-sample graph weights on the LDS path (solve(graph_params=...), solve(graph_sets=...), sweep with sigma keys,
mgadmm_solver_set_sample_graphs): sample b of a batch reads W_u, W_d and W_d^T of its own weight set -- all sets share the
instance's neighbour lists -- and equals the solve run alone by an instance CONSTRUCTED with that sample's (u_sigma, d_sigma):
bit for bit against those B = 1 solves (which run k_admm_lds; the batch runs k_admm_lds_pp), and within the project's float32
bound of 1e-5 of the float64 oracle built with the sample's own tables.

Fixture (tests/graph_sets_cases.py): the N = 30 graphs of g4_meta.npz with their distances, the 8 inputs of g5_batched.npz,
four sigma pairs {0.5, 1, 2, 4} x the fixture's sigma; samples 2j and 2j + 1 use pair j.  The census rows of test (h) come
from tests/lds_census.py at their own sizes."""
import ctypes as C

import numpy as np
import pytest
import torch

import graph_sets_cases as gc
import lds_census as lc
from conftest import admm_info_from, load_golden
from helpers import rel
from test_gpu_lds_census import _info as census_info, _inputs as census_inputs, _oracle as census_oracle, _product as census_product, env  # noqa: F401
from test_gpu_lds_census_units import _deciding_residuals
from test_gpu_sample_params import NAMES, ROWS, _solve

pytestmark = pytest.mark.gpu

FIXED_IT, F32_X_TOL = gc.FIXED_IT, gc.F32_X_TOL
SPATIAL = [i for i, (m, _) in enumerate(gc.CASES) if m != "line"]
SET_OF_SAMPLE = np.repeat(np.arange(4), 2)            # samples 2j, 2j + 1 -> pair j


def _blk(mode, abl, pair=None, **kw):
    """Instance constructed with `pair` (default: the fixture's own sigma, pair 1), fixed count, chunked schedule."""
    from mgadmm import _lib
    us, ds = gc.pairs()[1] if pair is None else pair
    blk = gc.instance(mode, abl, us, ds, path="lds", **kw)
    blk.max_ADMM_iter, blk.check_stop, blk.record_cg_coeffs = FIXED_IT, False, False
    return blk, _lib


def _gp(set_of_sample=SET_OF_SAMPLE, pairs=None):
    pairs = gc.pairs() if pairs is None else pairs
    return {"u_sigma": [pairs[j][0] for j in set_of_sample], "d_sigma": [pairs[j][1] for j in set_of_sample]}


def _unit(lib, blk):
    return lib.query(blk._solvers[(1, torch.float32)][0], lib.Q_LDS_UNIT)


def _weights_table(rows=ROWS):
    info = admm_info_from(gc.meta())
    return {nm: np.array([info[nm] * r[j] for r in rows]) for j, nm in enumerate(NAMES)}


def _assert_equals_solves_run_alone(mode, abl, batch, y, mask, samples, pair_of, table=None, prepare=None, what="sample"):
    """Sample b of `batch` against the B = 1 solve of an instance constructed with pair_of(b) (carrying row b of `table` as
    its scalars; `prepare(blk)` sets iteration limits), which runs k_admm_lds.  Zero tolerance."""
    made = {}
    for b in samples:
        pair = pair_of(b)
        if pair not in made:
            made[pair] = _blk(mode, abl, pair)[0]
            if prepare:
                prepare(made[pair])
        one_blk = made[pair]
        if table is not None:
            for nm in NAMES:
                setattr(one_blk, nm, float(table[nm][b]))
        one = _solve(one_blk, y[b:b + 1], abl, mask=None if mask is None else mask[b:b + 1])
        from mgadmm import _lib
        assert _unit(_lib, one_blk) == 0, (what, b)                       # the twin ran k_admm_lds
        nb = one["n_iters"]
        assert int(batch["n"][b]) == nb == int(one["n"][0]), (what, b, batch["n"][b], nb)
        for k in ("x", "zu", "zd", "phi"):
            if one[k] is not None:
                assert torch.equal(batch[k][b], one[k][0]), (what, b, k)
        assert set(batch["state"]) == set(one["state"])
        for k in one["state"]:
            assert torch.equal(batch["state"][k][b], one["state"][k][0]), (what, b, "state", k)
        assert np.array_equal(batch["mps"][:nb, :, b], one["mps"][:, :, 0]), (what, b, "metrics_per_sample")
        for cb, c1 in zip(batch["cg"], one["cg"]):
            assert np.array_equal(cb[:nb, b], c1[:, 0]), (what, b, "CG counts")
    for blk in made.values():
        blk.close()


# ---------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("i", range(len(gc.CASES)), ids=gc.IDS)
def test_batch_of_8_with_4_sigma_pairs(i):
    """Bitwise against eight B = 1 solves of instances constructed with each pair, and every sample within 1e-5 of the oracle
    built with its own tables.  The pairs discriminate: the oracle's solutions of one input under two pairs differ by at
    least 100 x 1e-5 -- measured (min over the 8 inputs and the 6 pairs of pairs, 40 iterations): knn-None 0.128, knn-DGLR
    0.137, physical-DGTV 0.115 at the starting factors {0.5, 1, 2, 4}.  The line-graph case of the file this test is
    modelled on has no spatial W_d tables: it must be refused (ValueError) and solve normally afterwards."""
    mode, abl = gc.CASES[i]
    blk, lib = _blk(mode, abl)
    y = gc.inputs()
    if mode == "line":
        with pytest.raises(ValueError, match="line-graph"):
            blk.solve(y, graph_params=_gp())
        assert blk._solvers == {}
        assert torch.isfinite(blk.solve(y)[0]).all()
        blk.close()
        return
    diff = gc.min_pair_difference(i)
    print(f"\n{mode}-{abl}: smallest oracle difference between two pairs {diff:.3e}")
    assert diff >= gc.MIN_DIFFERENCE, diff
    batch = _solve(blk, y, abl, graph_params=_gp())
    assert _unit(lib, blk) == 2
    assert batch["n_iters"] == FIXED_IT and (batch["n"] == FIXED_IT).all()
    pairs = gc.pairs()
    _assert_equals_solves_run_alone(mode, abl, batch, y, None, range(8), lambda b: pairs[SET_OF_SAMPLE[b]])
    xo = gc.oracle_solutions(i)
    for b in range(8):
        err = rel(batch["x"][b:b + 1], xo[SET_OF_SAMPLE[b], b:b + 1])
        print("sample", b, "pair", SET_OF_SAMPLE[b], "rel x against the oracle with its tables", err)
        assert err < F32_X_TOL, (b, err)
    # the table does not outlive the call: the next solve is the ordinary one of this instance (pair 1)
    plain = _solve(blk, y, abl)
    assert _unit(lib, blk) == 0 and torch.equal(plain["x"][2:4], batch["x"][2:4])
    blk.close()


def test_graph_sets_low_level_form_equals_graph_params():
    mode, abl = gc.CASES[0]
    blk, lib = _blk(mode, abl)
    y = gc.inputs()
    a = _solve(blk, y, abl, graph_params=_gp())
    sets = [blk._weight_tables(us, ds)[:2] for us, ds in gc.pairs()]
    b = _solve(blk, y, abl, graph_sets=[(u[0], d[0]) for u, d in sets], graph_of_sample=SET_OF_SAMPLE)      # (N, k) tables
    assert _unit(lib, blk) == 2 and torch.equal(a["x"], b["x"]) and np.array_equal(a["mps"], b["mps"])
    c = _solve(blk, y, abl, graph_params={"u_sigma": _gp()["u_sigma"]})          # d_sigma follows the instance
    one = _blk(mode, abl, (gc.pairs()[3][0], gc.pairs()[1][1]))[0]
    assert torch.equal(c["x"][7], _solve(one, y[7:8], abl)["x"][0])
    blk.close(); one.close()


# ---------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("i", [0, 3], ids=[gc.IDS[0], gc.IDS[3]])
def test_graph_table_and_weights_table_together(i):
    mode, abl = gc.CASES[i]
    blk, lib = _blk(mode, abl)
    y, table, pairs = gc.inputs(), _weights_table(), gc.pairs()
    batch = _solve(blk, y, abl, graph_params=_gp(), sample_params=table)
    assert _unit(lib, blk) == 2
    _assert_equals_solves_run_alone(mode, abl, batch, y, None, range(8), lambda b: pairs[SET_OF_SAMPLE[b]], table=table)
    blk.close()


# ---------------------------------------------------------------------------------------------------------- (c)
def test_per_sample_stopping(env):
    """ADMM_tol by lc.pick_admm_tol on the deciding residuals of the eight B = 1 solves: no residual within 1 % of it, the
    samples stop at different iterations and in different launches of 4."""
    env.setenv("MGADMM_LDS_CHUNK", str(lc.UNIT_CHUNK))
    mode, abl = gc.CASES[0]
    K, y, pairs = FIXED_IT, gc.inputs(), gc.pairs()
    res = []
    for b in range(8):
        one = _blk(mode, abl, pairs[SET_OF_SAMPLE[b]])[0]
        res.append(_deciding_residuals(_solve(one, y[b:b + 1], abl)["mps"], abl))
        one.close()
    tol, n_first = lc.pick_admm_tol(np.stack(res), K)
    print("\nADMM_tol", tol, "first crossings", n_first)
    blk, lib = _blk(mode, abl, admm_convergence="per_sample")
    blk.ADMM_tol, blk.check_stop = tol, True
    batch = _solve(blk, y, abl, graph_params=_gp())
    assert _unit(lib, blk) == 2 and batch["n"].tolist() == n_first and batch["n_iters"] == max(n_first)

    def prepare(one):
        one.ADMM_tol, one.check_stop = tol, True
    _assert_equals_solves_run_alone(mode, abl, batch, y, None, range(8), lambda b: pairs[SET_OF_SAMPLE[b]], prepare=prepare)
    blk.close()


# ---------------------------------------------------------------------------------------------------------- (d)
def test_interpolation_with_a_mask():
    m = gc.meta()
    xs = load_golden("g5_batched.npz")["x"].astype(np.float64)
    mask64 = np.broadcast_to(m["mask"].astype(np.float64), xs.shape).copy()
    y, mask = torch.from_numpy((xs * mask64).astype(np.float32)), torch.from_numpy(mask64.astype(np.float32))
    mode, abl = gc.CASES[0]
    blk, lib = _blk(mode, abl)
    batch = _solve(blk, y, abl, mask=mask, graph_params=_gp())
    assert _unit(lib, blk) == 2
    pairs = gc.pairs()
    _assert_equals_solves_run_alone(mode, abl, batch, y, mask, range(8), lambda b: pairs[SET_OF_SAMPLE[b]])
    blk.close()


# ---------------------------------------------------------------------------------------------------------- (e)
def test_resume_in_the_middle_of_the_solve():
    mode, abl = gc.CASES[0]
    blk, _ = _blk(mode, abl)
    y = gc.inputs()
    full = _solve(blk, y, abl, graph_params=_gp())
    blk.max_ADMM_iter = 15
    first = _solve(blk, y, abl, graph_params=_gp())
    blk.max_ADMM_iter = FIXED_IT - 15
    second = _solve(blk, y, abl, graph_params=_gp(), warm_start=first["state"])
    assert second["n_iters"] == FIXED_IT - 15
    for k in full["state"]:
        assert torch.equal(second["state"][k], full["state"][k]), k
    assert np.array_equal(second["mps"], full["mps"][15:])
    blk.close()


# ---------------------------------------------------------------------------------------------------------- (f)
def test_synchronous_schedule_equals_the_chunked_one():
    mode, abl = gc.CASES[0]
    blk, lib = _blk(mode, abl)
    y = gc.inputs()
    assert lib.query(blk._solver(1, torch.float32, 8)[0], lib.Q_LDS_CHUNK) > 1
    chunked = _solve(blk, y, abl, graph_params=_gp())
    blk.record_cg_coeffs = True               # alpha / beta of every CG iteration: one iteration per launch, host in between
    sync = _solve(blk, y, abl, graph_params=_gp())
    assert _unit(lib, blk) == 2 and len(blk.alpha_x) == FIXED_IT
    for k in chunked["state"]:
        assert torch.equal(sync["state"][k], chunked["state"][k]), k
    assert np.array_equal(sync["mps"], chunked["mps"])
    for a, b in zip(sync["cg"], chunked["cg"]):
        assert np.array_equal(a, b)
    blk.close()


# ---------------------------------------------------------------------------------------------------------- (g)
def test_large_batch_of_128_sets():
    """B = 1024 = 128 sets x 8 windows (window index fastest): u_sigma rises from 0.5 to 4 x the fixture's sigma over the
    sets while d_sigma falls from 4 to 0.5 x."""
    mode, abl = gc.CASES[0]
    P, W, s = 128, 8, float(gc.meta()["sigma"])
    f = 0.5 * 8.0 ** (np.arange(P) / (P - 1))
    pairs = [(float(s * f[j]), float(s * f[P - 1 - j])) for j in range(P)]
    sos = np.repeat(np.arange(P), W)
    y = gc.inputs().repeat(P, 1, 1, 1)
    blk, lib = _blk(mode, abl)
    batch = _solve(blk, y, abl, graph_params=_gp(sos, pairs))
    assert _unit(lib, blk) == 2 and torch.isfinite(batch["x"]).all()
    _assert_equals_solves_run_alone(mode, abl, batch, y, None, [0, P * W // 2, P * W - 1], lambda b: pairs[sos[b]])
    assert not torch.equal(batch["x"][0], batch["x"][W])           # neighbouring sets give different solutions
    blk.close()


def test_sweep_with_sigma_keys():
    mode, abl = gc.CASES[0]
    blk, lib = _blk(mode, abl)
    y, s = gc.inputs()[:4], float(gc.meta()["sigma"])
    grid = {"u_sigma": [0.5 * s, 2 * s], "mu_u": [0.5, 1], "d_sigma": [s, 4 * s]}
    x, n, sets = blk.sweep(y, grid)
    assert tuple(x.shape) == (8, 4, 24, 30, 1) and (n == FIXED_IT).all() and len(sets) == 8
    for p, w in [(0, 0), (3, 1), (5, 2), (7, 3)]:
        one = _blk(mode, abl, (sets[p]["u_sigma"], sets[p]["d_sigma"]))[0]
        one.mu_u = float(sets[p]["mu_u"])
        assert torch.equal(x[p, w], one.solve(y[w:w + 1])[0][0]), (p, w)
        one.close()
    blk.close()


# ---------------------------------------------------------------------------------------------------------- (h)
CENSUS_ROWS = [lc.uni(8, 1024, True, 2), lc.uni(8, 1024, True, -1), lc.inst(3, False, 1024, False), lc.inst(12, False, 640, True)]
CENSUS_K, CENSUS_B, CENSUS_FACTORS = 12, 6, (1.0, 0.5, 2.0)


@pytest.mark.parametrize("expect", CENSUS_ROWS, ids=[lc.row_id(dict(expect=e)) for e in CENSUS_ROWS])
def test_census_rows_with_three_sets(expect, env):
    """Uniform rows with a compile-time tail (TP 2), uniform rows with a run-time tail, a generic instance with ragged rows and
    a single-buffer instance: three sets (the row's default sigma x 1, 0.5, 2) at B = 6, launches of 4 iterations."""
    from mgadmm import _lib
    from mgadmm import utils as mu
    r = dict(next(r for r in lc.CENSUS if r["expect"] == expect), B=CENSUS_B)
    for k, v in r["env"].items():
        env.setenv(k, v)
    env.setenv("MGADMM_LDS_CHUNK", str(lc.UNIT_CHUNK))
    abl, info = r["abl"], census_info(r["N"], r["T"])
    y, mask = census_inputs(r)
    yt, mt = torch.from_numpy(y), None if mask is None else torch.from_numpy(mask)
    blk = census_product(r, info, path="lds")
    blk.max_ADMM_iter, blk.check_stop = CENSUS_K, False
    s0 = float(mu._sigma_default(blk.connect_list, blk.dist_list))
    pairs = [(f * s0, f * s0) for f in CENSUS_FACTORS]
    sos = np.arange(CENSUS_B) % 3
    batch = _solve(blk, yt, abl, mask=mt, graph_params=_gp(sos, pairs))
    h = blk._solvers[(1, torch.float32)][0]
    assert (_lib.query(h, _lib.Q_LDS_UNIT), _lib.lds_instance(h)) == (2, expect)
    assert _lib.query(h, _lib.Q_LDS_CHUNK) == lc.UNIT_CHUNK and batch["n_iters"] == CENSUS_K
    twins = []
    for us, ds in pairs:
        t = census_product(r, info, path="lds", u_sigma=us, d_sigma=ds)
        t.max_ADMM_iter, t.check_stop = CENSUS_K, False
        twins.append(t)
    assert torch.equal(twins[0].u_ew, blk.u_ew) and torch.equal(twins[0].d_ew, blk.d_ew)       # factor 1 is the default sigma
    for b in range(CENSUS_B):
        t = twins[sos[b]]
        one = _solve(t, yt[b:b + 1], abl, mask=None if mt is None else mt[b:b + 1])
        ht = t._solvers[(1, torch.float32)][0]
        assert (_lib.query(ht, _lib.Q_LDS_UNIT), _lib.lds_instance(ht)) == (0, expect), b
        assert torch.equal(batch["x"][b], one["x"][0]), b
        for k in one["state"]:
            assert torch.equal(batch["state"][k][b], one["state"][k][0]), (b, k)
        assert np.array_equal(batch["mps"][:, :, b], one["mps"][:, :, 0]), b
        for cb, c1 in zip(batch["cg"], one["cg"]):
            assert np.array_equal(cb[:, b], c1[:, 0]), b
    b = CENSUS_B - 1
    o = census_oracle(r, twins[sos[b]], info)
    xo = o.combined_loop(y[b:b + 1].astype(np.float64), mask=None if mask is None else mask[b:b + 1], n_iters=CENSUS_K)
    err = rel(batch["x"][b:b + 1], xo)
    print(f"\n{expect}: sample {b} (sigma x {CENSUS_FACTORS[sos[b]]}) against the oracle with its tables: {err:.2e}")
    assert err < F32_X_TOL, err
    for t in twins:
        t.close()
    blk.close()


# ---------------------------------------------------------------------------------------------------------- (i)
def _expect_refused(blk, y, lib, reason, code=None, **kw):
    blk._reset_history()
    kw = kw or dict(graph_params=_gp())
    with pytest.raises(lib.MgadmmError) as e:
        blk.solve(y, **kw)
    assert e.value.code == (lib.ERR_UNSUPPORTED if code is None else code), e.value
    assert "sample_graphs" in str(e.value) and reason in str(e.value), e.value
    assert blk.p_res_list == []                                  # nothing ran
    x = blk.solve(y)[0]                                          # the same instance still solves normally
    assert torch.isfinite(x).all() and len(blk.p_res_list) > 0


def test_refused_on_the_streaming_path():
    blk, lib = _blk("knn", "None")
    blk.path, blk.max_ADMM_iter = "stream", 3
    _expect_refused(blk, gc.inputs(), lib, "MGADMM_PATH_STREAM")
    blk.close()


def test_refused_in_float64():
    from mgadmm import _lib as lib
    blk = gc.instance("knn", "None", *gc.pairs()[1], compute_dtype=torch.float64)
    blk.max_ADMM_iter, blk.check_stop = 3, False
    _expect_refused(blk, gc.inputs().double(), lib, "float64")
    blk.close()


def test_refused_with_batch_max_cg_convergence():
    from mgadmm import _lib as lib
    blk = gc.instance("knn", "None", *gc.pairs()[1], cg_convergence="batch_max")
    blk.max_ADMM_iter, blk.check_stop = 3, False
    _expect_refused(blk, gc.inputs(), lib, "batch_max")
    blk.close()


def test_refused_for_a_line_graph():
    blk, lib = _blk("line", "None")
    blk.max_ADMM_iter = 3
    y = gc.inputs()
    for kw in (dict(graph_params=_gp()), dict(graph_sets=[(blk.u_ew, blk.d_ew)], graph_of_sample=[0] * 8)):
        with pytest.raises(ValueError, match="line-graph"):
            blk.solve(y, **kw)
    # and straight through the C ABI: a band graph as a weight set of a band solver
    x = blk.solve(y)[0]
    h = blk._solvers[(1, torch.float32)][0]
    g = blk._graphs[1][0]
    sos = np.zeros(8, dtype=np.int32)
    rc = lib.lib.mgadmm_solver_set_sample_graphs(h, 1, (C.c_void_p * 1)(g.handle), sos.ctypes.data_as(C.POINTER(C.c_int32)), 8)
    assert rc == lib.ERR_UNSUPPORTED and b"band graph" in lib.lib.mgadmm_last_error()
    assert torch.equal(blk.solve(y)[0], x)
    blk.close()


def test_refused_with_the_whole_batch_stop_test():
    blk, lib = _blk("knn", "None")
    blk.check_stop, blk.ADMM_tol, blk.max_ADMM_iter = True, 1e-6, 5
    assert blk.admm_convergence == "whole_batch"
    _expect_refused(blk, gc.inputs(), lib, "whole_batch")
    blk.close()


def test_pattern_mismatch_set_index_and_batch_size_through_the_c_abi():
    blk, lib = _blk("knn", "None")
    y = gc.inputs()
    blk.max_ADMM_iter = 3
    x_plain = blk.solve(y)[0]                                    # the solver exists, max_batch = 8
    h = blk._solvers[(1, torch.float32)][0]
    setg = lib.lib.mgadmm_solver_set_sample_graphs
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    err = lambda: lib.lib.mgadmm_last_error().decode()
    own = blk._graphs[1][0]
    arr = lambda *gs: (C.c_void_p * len(gs))(*[g.handle for g in gs])
    zeros8 = np.zeros(8, dtype=np.int32)

    # pattern mismatch: the same table with one neighbour of node 3 replaced -> the set's W_d^T rows differ
    cl = blk.connect_list.clone()
    cl[3, 4] = next(j for j in range(30) if j not in cl[3].tolist())
    saved, blk.connect_list = blk.connect_list, cl
    other = blk._make_graph(1, blk.u_ew, blk.d_ew)
    blk.connect_list = saved
    assert setg(h, 2, arr(own, other), ip(zeros8), 8) == lib.ERR_UNSUPPORTED
    msg = err()
    assert "sample_graphs set 1" in msg and "topology" in msg, msg
    field = msg.split(" -- ")[1].split(":")[0]
    assert field in ("instance", "tail_pairs", "npos", "en_u", "en_d", "lead_t", "tail_t", "node_of_row", "row_of_node"), msg
    print("\npattern mismatch reported as:", msg)
    other.close()
    assert torch.equal(blk.solve(y)[0], x_plain)

    # set index out of range; null handle; B > max_batch
    bad = zeros8.copy(); bad[5] = 1
    assert setg(h, 1, arr(own), ip(bad), 8) == lib.ERR_INVALID and "set_of_sample[5]" in err()
    assert setg(h, 1, (C.c_void_p * 1)(None), ip(zeros8), 8) == lib.ERR_INVALID and "graphs[0]" in err()
    assert setg(h, 1, arr(own), ip(np.zeros(9, dtype=np.int32)), 9) == lib.ERR_INVALID and "max_batch" in err()
    with pytest.raises(ValueError, match="out of range"):
        blk.solve(y, graph_sets=[(blk.u_ew, blk.d_ew)], graph_of_sample=[0, 0, 0, 0, 0, 0, 0, 1])
    assert torch.equal(blk.solve(y)[0], x_plain)

    # B mismatch: a table of 4 samples, a solve of 8
    assert setg(h, 1, arr(own), ip(np.zeros(4, dtype=np.int32)), 4) == lib.OK
    blk._reset_history()
    with pytest.raises(lib.MgadmmError) as e:
        blk.solve(y)
    assert e.value.code == lib.ERR_INVALID and "sample_graphs" in str(e.value) and "4 samples" in str(e.value) and blk.p_res_list == []
    assert setg(h, 0, None, None, 0) == lib.OK
    assert torch.equal(blk.solve(y)[0], x_plain)
    blk.close()
