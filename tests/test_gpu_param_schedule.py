"""Per-iteration ADMM weights (solve(param_schedule=..., schedule_start=...), sweep(schedules=...),
mgadmm_solver_set_param_schedule): iteration k of a solve reads row min(first_row + k, n_rows - 1) of a table of the six
weights, shared by the batch or one column per sample.  A scheduled solve of K iterations equals, bit for bit, the CHAIN:
K solves of one iteration, resumed with warm_start=, the row's six doubles assigned as scalars (B = 1 solves of the product,
which run k_admm_lds; the scheduled batch runs k_admm_lds_pp, up to 16 iterations per launch), and lies within the project's
float32 tolerances of the float64 twin of tests/param_schedule_cases.py.

Fixture (tests/param_schedule_cases.py): tables of g4_meta.npz, the 8 inputs of g5_batched.npz, four cases; 12 rows, K = 20
iterations: the clamp to the last row and the launch boundary 16 + 4 are both hit."""
import functools

import numpy as np
import pytest
import torch

import lds_census as lc
import param_schedule_cases as pc
from helpers import check_windows, make_product, rel
from test_gpu_lds_census import _info as census_info, _inputs as census_inputs, _product as census_product, env  # noqa: F401
from test_gpu_lds_census_units import _deciding_residuals
from test_gpu_sample_params import _solve

pytestmark = pytest.mark.gpu

NAMES, CASES, IDS, K = pc.NAMES, pc.CASES, pc.IDS, pc.K
F32_X_TOL, F32_HIST_RTOL = pc.F32_X_TOL, pc.F32_HIST_RTOL
RAMP_SAMPLES = [b for b, t in enumerate(pc.TAU) if t != 1.0 and b not in pc.MU_SAMPLES]


def _blk(mode, abl, **kw):
    from mgadmm import _lib
    kw.setdefault("path", "lds")
    blk = make_product(pc.meta(), mode, ablation=abl, **kw)
    blk.max_ADMM_iter, blk.check_stop = K, False
    blk.record_cg_coeffs = False              # the chunked schedule (several iterations per launch)
    return blk, _lib


def _handle(blk, dtype=torch.float32):
    return blk._solvers[(1, dtype)][0]


def _unit(lib, blk):
    return lib.query(_handle(blk), lib.Q_LDS_UNIT)


def _chain(blk, y, abl, weights_of, n_it, stop_tol=None):
    """n_it solves of ONE iteration by `blk`, each resumed from the state of the one before (the first from the initial
    guess), with weights_of(it) -- the six doubles of the iteration -- assigned as the instance's scalars.  No table of
    any kind: on the LDS path these launches run k_admm_lds.  stop_tol: the chain ends after the first iteration whose
    deciding residual (B = 1) is below it.  Returns the snapshot of the last solve with the rows of metrics_per_sample and
    the CG counts of all iterations, and `steps`, the snapshot after every iteration."""
    blk.max_ADMM_iter, blk.check_stop = 1, False
    state, steps = None, []
    for it in range(n_it):
        for nm, v in weights_of(it).items():
            setattr(blk, nm, v)
        steps.append(_solve(blk, y, abl, warm_start=state))
        assert steps[-1]["n_iters"] == 1
        state = steps[-1]["state"]
        if stop_tol is not None and _deciding_residuals(steps[-1]["mps"], abl)[0] < stop_tol:
            break
    out = dict(steps[-1])
    out["mps"] = np.concatenate([s["mps"] for s in steps])
    out["cg"] = [np.concatenate([s["cg"][w] for s in steps]) for w in range(len(steps[0]["cg"]))]
    out["n_iters"], out["steps"] = len(steps), steps
    return out


def _assert_sample_equals(batch, b, one, what=""):
    """Sample b of a batch result against a B = 1 result (a chain): x, the state, the per-sample metrics and the CG counts of
    every iteration.  Zero tolerance: the kernels are compiled from one source and read the same eight floats."""
    nb = one["n_iters"]
    assert int(batch["n"][b]) == nb, (what, b, batch["n"][b], nb)
    for k in ("x", "zu", "zd", "phi"):
        if one[k] is not None:
            assert torch.equal(batch[k][b], one[k][0]), (what, b, k)
    assert set(batch["state"]) == set(one["state"])
    for k in one["state"]:
        assert torch.equal(batch["state"][k][b], one["state"][k][0]), (what, b, "state", k)
    assert np.array_equal(batch["mps"][:nb, :, b], one["mps"][:, :, 0]), (what, b, "metrics_per_sample")
    for cb, c1 in zip(batch["cg"], one["cg"]):
        assert np.array_equal(cb[:nb, b], c1[:, 0]), (what, b, "CG counts")


def _assert_same(a, b, what=""):
    for k in ("x", "zu", "zd", "phi"):
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), (what, k)
    for k in a["state"]:
        assert torch.equal(a["state"][k], b["state"][k]), (what, "state", k)
    assert np.array_equal(a["n"], b["n"]) and a["n_iters"] == b["n_iters"], what
    assert np.array_equal(a["mps"], b["mps"]), (what, "metrics_per_sample")
    for ca, cb in zip(a["cg"], b["cg"]):
        assert np.array_equal(ca, cb), (what, "CG counts")


@functools.lru_cache(maxsize=None)
def _batch(i):
    """The scheduled batch of 8 of case i, default launch shape (asserted: several iterations per launch, k_admm_lds_pp)."""
    mode, abl = CASES[i]
    blk, lib = _blk(mode, abl)
    out = _solve(blk, pc.inputs(), abl, param_schedule=pc.table())
    assert lib.query(_handle(blk), lib.Q_LDS_CHUNK) > 1 and _unit(lib, blk) == 2
    assert out["n_iters"] == K and (out["n"] == K).all()
    blk.close()
    return out


@functools.lru_cache(maxsize=None)
def _chains(i):
    """The chains of the 8 samples of case i (asserted: k_admm_lds)."""
    mode, abl = CASES[i]
    one_blk, lib = _blk(mode, abl)
    y, tab = pc.inputs(), pc.table()
    out = [_chain(one_blk, y[b:b + 1], abl, lambda it, b=b: pc.scalars_of(tab, b, it), K) for b in range(8)]
    assert _unit(lib, one_blk) == 0
    one_blk.close()
    return out


# ---------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_scheduled_batch_equals_the_chain_bit_for_bit(i, env):
    batch, chains = _batch(i), _chains(i)
    for b in range(8):
        assert chains[b]["n_iters"] == K
        _assert_sample_equals(batch, b, chains[b], IDS[i])


# ---------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_every_sample_matches_its_float64_twin(i, env):
    """The project's own tolerances: 1e-5 on x, 1e-3 on the history, +-1 on the CG counts.  The twin discriminates by 50 x
    (one row off) and 500 x (no schedule) the x tolerance: tests/test_param_schedule_cpu.py."""
    mode, abl = CASES[i]
    blk, _ = _blk(mode, abl)
    blk._reset_history()
    x = blk.solve(pc.inputs(), per_sample_history=True, param_schedule=pc.table())[0]
    twins = pc.twin_solutions(i)
    for b in range(8):
        xo, o = twins[b]
        print("sample", b, "rel x against the twin", rel(x[b:b + 1], xo))
        check_windows(f"{IDS[i]} sample {b}", blk, x, [b], o, xo, xtol=F32_X_TOL, htol=F32_HIST_RTOL, slack=1, abl=abl)
    blk.close()


def test_streaming_float64_shared_form_matches_the_twin(env):
    mode, abl = CASES[0]
    sched = pc.column(pc.table(), 3)
    blk = make_product(pc.meta(), mode, ablation=abl, compute_dtype=torch.float64)
    blk.max_ADMM_iter, blk.check_stop = K, False
    y = pc.inputs().double()
    blk._reset_history()
    x = blk.solve(y, param_schedule=sched)[0]
    o = pc.scheduled_oracle(mode, abl, sched)
    xo = o.combined_loop(y.numpy(), n_iters=K)
    err = rel(x, xo)
    print("float64 streaming path against the twin", err)
    assert err < 1e-10, err
    for nm in ("CG_iter_x", "CG_iter_zu", "CG_iter_zd"):
        assert np.array_equal(torch.stack(getattr(blk, nm)).numpy(), np.array(getattr(o.hist, nm)).reshape(K, -1)), nm
    # the schedule matters there too
    x0 = blk.solve(y)[0]
    assert rel(x, x0) > 10 * F32_X_TOL
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_other_launch_shapes_give_the_same_bits(i, env):
    mode, abl = CASES[i]
    ref = _batch(i)                           # (the default launch shape: before the switch below)
    env.setenv("MGADMM_LDS_CHUNK", "4")
    blk, lib = _blk(mode, abl)
    four = _solve(blk, pc.inputs(), abl, param_schedule=pc.table())
    assert lib.query(_handle(blk), lib.Q_LDS_CHUNK) == 4 and _unit(lib, blk) == 2
    _assert_same(four, ref, "launches of 4")
    blk.record_cg_coeffs = True               # the synchronous schedule: one iteration per launch
    sync = _solve(blk, pc.inputs(), abl, param_schedule=pc.table())
    assert _unit(lib, blk) == 2
    _assert_same(sync, ref, "synchronous schedule")
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 4
def test_clamp_and_resume(env):
    mode, abl = CASES[0]
    blk, _ = _blk(mode, abl)
    y, tab, full = pc.inputs(), pc.table(), _batch(0)
    _assert_same(_solve(blk, y, abl, param_schedule=pc.padded(tab, K)), full, "12 rows against 20 rows padded by hand")
    blk.max_ADMM_iter = 8
    first = _solve(blk, y, abl, param_schedule=tab)
    blk.max_ADMM_iter = K - 8
    second = _solve(blk, y, abl, param_schedule=tab, schedule_start=8, warm_start=first["state"])
    assert second["n_iters"] == K - 8
    for k in ("x", "zu", "zd", "phi"):
        assert torch.equal(second[k], full[k]), k
    for k in full["state"]:
        assert torch.equal(second["state"][k], full["state"][k]), k
    assert np.array_equal(np.concatenate([first["mps"], second["mps"]]), full["mps"])
    blk.max_ADMM_iter = K
    late = _solve(blk, y, abl, param_schedule=tab, schedule_start=1)
    assert torch.equal(late["x"][0], full["x"][0])                     # sample 0: equal rows
    for b in RAMP_SAMPLES:
        d = rel(late["x"][b:b + 1], full["x"][b:b + 1])
        print("sample", b, "schedule_start 1 against 0:", d)
        assert d > 10 * F32_X_TOL, (b, d)
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("path", ["lds", "stream"])
def test_a_schedule_of_equal_rows_is_the_ordinary_solve(path, env):
    mode, abl = CASES[0]
    blk, lib = _blk(mode, abl, path=path)
    y, inf = pc.inputs(), pc.info()
    plain = _solve(blk, y, abl)
    if path == "lds":
        assert _unit(lib, blk) == 0
        inst = lib.lds_instance(_handle(blk))
        same = _solve(blk, y, abl, param_schedule={nm: np.full((pc.N_ROWS, 8), float(inf[nm])) for nm in NAMES})
        assert _unit(lib, blk) == 2 and lib.lds_instance(_handle(blk)) == inst
        _assert_same(same, plain, "per-sample form")
    shared = _solve(blk, y, abl, param_schedule={nm: np.full(pc.N_ROWS, float(inf[nm])) for nm in NAMES})
    _assert_same(shared, plain, "shared form")
    part = _solve(blk, y, abl, param_schedule={"mu_u": np.full(3, float(inf["mu_u"]))})      # the other five follow the scalars
    _assert_same(part, plain, "one name")
    after = _solve(blk, y, abl)                                        # cleared after the call
    if path == "lds":
        assert _unit(lib, blk) == 0
    _assert_same(after, plain, "after")
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 6
def test_per_sample_form_stops_every_sample_on_its_own_residuals(env):
    """ADMM_tol by lc.pick_admm_tol on the chains' deciding residuals: no residual within 1 % of it, the samples stop at
    different iterations and in different launches of 4."""
    mode, abl = CASES[0]
    chains = _chains(0)
    env.setenv("MGADMM_LDS_CHUNK", str(lc.UNIT_CHUNK))
    tol, n_first = lc.pick_admm_tol(np.stack([_deciding_residuals(c["mps"], abl) for c in chains]), K)
    print("\nADMM_tol", tol, "first crossings", n_first)
    blk, lib = _blk(mode, abl, admm_convergence="per_sample")
    blk.ADMM_tol, blk.check_stop = tol, True
    batch = _solve(blk, pc.inputs(), abl, param_schedule=pc.table())
    assert _unit(lib, blk) == 2 and batch["n"].tolist() == n_first and batch["n_iters"] == max(n_first)
    for b in range(8):
        nb = n_first[b]
        step = chains[b]["steps"][nb - 1]                              # the chain run until its own residuals pass
        assert _deciding_residuals(step["mps"], abl)[0] < tol and all(
            _deciding_residuals(s["mps"], abl)[0] >= tol for s in chains[b]["steps"][:nb - 1])
        assert torch.equal(batch["x"][b], step["x"][0]), b
        for k in step["state"]:
            assert torch.equal(batch["state"][k][b], step["state"][k][0]), (b, k)
        assert np.array_equal(batch["mps"][:nb, :, b], chains[b]["mps"][:nb, :, 0]), b
    blk.close()


def _whole_batch_residuals(o):
    return np.array([max(max(p), max(d)) for p, d in zip(o.hist.p_res_list, o.hist.d_res_list)])


def test_shared_form_stops_on_the_whole_batch_test(env):
    """The tolerance: the geometric mean of two consecutive whole-batch residuals of the twin, where they fall the most (so
    that no stop is a rounding decision; asserted: more than 5 % away from every residual up to the stop)."""
    mode, abl = CASES[0]
    sched = pc.column(pc.table(), 3)
    y = pc.inputs()
    o = pc.scheduled_oracle(mode, abl, sched)
    o.combined_loop(y.double().numpy(), n_iters=K)
    r = _whole_batch_residuals(o)
    cand = [k for k in range(4, K - 1) if (r[:k] > np.sqrt(r[k - 1] * r[k])).all()]
    k = max(cand, key=lambda k: r[k - 1] / r[k])
    tol = float(np.sqrt(r[k - 1] * r[k]))
    assert np.abs(np.log(r[:k + 1] / tol)).min() > np.log(1.05), (k, r)
    twin = pc.scheduled_oracle(mode, abl, sched)
    twin.ADMM_tol, twin.max_ADMM_iter = tol, K
    twin.combined_loop(y.double().numpy())
    n_twin = len(twin.hist.p_res_list)
    assert n_twin == k + 1
    print("\nADMM_tol", tol, "the twin stops after", n_twin)
    blk, lib = _blk(mode, abl)
    blk.ADMM_tol, blk.check_stop = tol, True
    dev = _solve(blk, y, abl, param_schedule=sched)                    # the device stop test, launches enqueued ahead
    assert _unit(lib, blk) == 2 and dev["n_iters"] == n_twin
    blk.close()
    env.setenv("MGADMM_LDS_ASYNC", "0")
    blk, lib = _blk(mode, abl)
    blk.ADMM_tol, blk.check_stop = tol, True
    sync = _solve(blk, y, abl, param_schedule=sched)
    assert _unit(lib, blk) == 2 and sync["n_iters"] == n_twin
    assert torch.equal(dev["x"], sync["x"]) and np.array_equal(dev["mps"], sync["mps"])
    for k2 in sync["state"]:
        assert torch.equal(dev["state"][k2], sync["state"][k2]), k2
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 7
def test_streaming_float32_shared_form_equals_its_chain(env):
    mode, abl = CASES[0]
    tab, y = pc.table(), pc.inputs()
    blk, _ = _blk(mode, abl, path="stream")
    sched = _solve(blk, y, abl, param_schedule=pc.column(tab, 3))
    assert sched["n_iters"] == K
    one_blk, _ = _blk(mode, abl, path="stream")
    chain = _chain(one_blk, y, abl, lambda it: pc.scalars_of(tab, 3, it), K)
    for k in ("x", "zu", "zd", "phi"):
        assert torch.equal(sched[k], chain[k]), k
    for k in chain["state"]:
        assert torch.equal(sched["state"][k], chain["state"][k]), k
    assert np.array_equal(sched["mps"], chain["mps"])
    for a, b in zip(sched["cg"], chain["cg"]):
        assert np.array_equal(a, b)
    assert rel(sched["x"], _solve(blk, y, abl)["x"]) > 10 * F32_X_TOL          # the schedule matters
    blk.close(); one_blk.close()


# ---------------------------------------------------------------------------------------------------------- 8
def test_more_samples_than_compute_units(env):
    """B = 1024 = 128 schedules x 8 windows (window index fastest): schedule j ramps the rhos by 0.95 + 0.25 j / 127 per row."""
    mode, abl = CASES[0]
    P, W = 128, 8
    tab = pc.table(tau=tuple(np.repeat(0.95 + 0.25 * np.arange(P) / (P - 1), W)))
    assert tab["rho"].shape == (pc.N_ROWS, P * W)
    y = pc.inputs().repeat(P, 1, 1, 1)
    blk, lib = _blk(mode, abl)
    batch = _solve(blk, y, abl, param_schedule=tab)
    assert _unit(lib, blk) == 2 and batch["n_iters"] == K
    one_blk, _ = _blk(mode, abl)
    for b in (0, 512, 1023):
        _assert_sample_equals(batch, b, _chain(one_blk, y[b:b + 1], abl, lambda it, b=b: pc.scalars_of(tab, b, it), K), "B = 1024")
    blk.close(); one_blk.close()


# ---------------------------------------------------------------------------------------------------------- 9
CENSUS_ROWS = [lc.uni(8, 1024, True, 2), lc.uni(8, 1024, True, -1), lc.inst(3, False, 1024, False), lc.inst(12, False, 640, True),
               lc.inst(2, True, 1024, False)]
CENSUS_K, CENSUS_B, CENSUS_ROWS_N = 12, 6, 8


@pytest.mark.parametrize("expect", CENSUS_ROWS, ids=[lc.row_id(dict(expect=e)) for e in CENSUS_ROWS])
def test_census_rows(expect, env):
    """Uniform rows with a compile-time tail (TP 2), uniform rows with a run-time tail, a generic instance with ragged rows, a
    single-buffer instance and a band instance: B = 6, an 8-row per-sample schedule (sample b ramps the rhos by
    0.9 + 0.06 b per row and mu_u by 1.02 per row), 12 iterations in launches of 4."""
    from mgadmm import _lib
    r = dict(next(r for r in lc.CENSUS if r["expect"] == expect), B=CENSUS_B)
    for k, v in r["env"].items():
        env.setenv(k, v)
    env.setenv("MGADMM_LDS_CHUNK", str(lc.UNIT_CHUNK))
    abl, info = r["abl"], census_info(r["N"], r["T"])
    y, mask = census_inputs(r)
    yt, mt = torch.from_numpy(y), None if mask is None else torch.from_numpy(mask)
    rows = np.arange(CENSUS_ROWS_N, dtype=np.float64)[:, None]
    tab = {nm: float(info[nm]) * (0.9 + 0.06 * np.arange(CENSUS_B)[None, :]) ** rows for nm in NAMES[:3]}
    tab["mu_u"] = float(info["mu_u"]) * 1.02 ** rows * np.ones((1, CENSUS_B))
    blk = census_product(r, info, path="lds")
    blk.max_ADMM_iter, blk.check_stop = CENSUS_K, False
    batch = _solve(blk, yt, abl, mask=mt, param_schedule=tab)
    h = _handle(blk)
    assert (_lib.query(h, _lib.Q_LDS_UNIT), _lib.lds_instance(h)) == (2, expect)
    assert _lib.query(h, _lib.Q_LDS_CHUNK) == lc.UNIT_CHUNK and batch["n_iters"] == CENSUS_K
    one_blk = census_product(r, info, path="lds")
    for b in (0, 3, 5):
        def run(it, b=b):
            return {nm: float(v[min(it, CENSUS_ROWS_N - 1), b]) for nm, v in tab.items()}
        state, steps = None, []
        one_blk.max_ADMM_iter, one_blk.check_stop = 1, False
        for it in range(CENSUS_K):
            for nm, v in run(it).items():
                setattr(one_blk, nm, v)
            steps.append(_solve(one_blk, yt[b:b + 1], abl, mask=None if mt is None else mt[b:b + 1], warm_start=state))
            state = steps[-1]["state"]
        ht = _handle(one_blk)
        assert (_lib.query(ht, _lib.Q_LDS_UNIT), _lib.lds_instance(ht)) == (0, expect), b
        last = steps[-1]
        assert torch.equal(batch["x"][b], last["x"][0]), b
        for k in last["state"]:
            assert torch.equal(batch["state"][k][b], last["state"][k][0]), (b, k)
        assert np.array_equal(batch["mps"][:, :, b], np.concatenate([s["mps"] for s in steps])[:, :, 0]), b
        for w, cb in enumerate(batch["cg"]):
            assert np.array_equal(cb[:, b], np.concatenate([s["cg"][w] for s in steps])[:, 0]), b
    blk.close(); one_blk.close()


# ---------------------------------------------------------------------------------------------------------- 10
def _expect_refused(blk, y, lib, reason, code=None, **kw):
    blk._reset_history()
    kw = kw or dict(param_schedule=pc.table())
    with pytest.raises(lib.MgadmmError) as e:
        blk.solve(y, **kw)
    assert e.value.code == (lib.ERR_UNSUPPORTED if code is None else code), e.value
    assert "param_schedule" in str(e.value) and reason in str(e.value), e.value
    assert blk.p_res_list == []                                  # nothing ran
    x = blk.solve(y)[0]                                          # the same instance still solves normally
    assert torch.isfinite(x).all() and len(blk.p_res_list) > 0


def test_per_sample_form_refused_on_the_streaming_path(env):
    blk, lib = _blk("knn", "None", path="stream")
    blk.max_ADMM_iter = 3
    _expect_refused(blk, pc.inputs(), lib, "MGADMM_PATH_STREAM")
    blk.close()


def test_per_sample_form_refused_in_float64(env):
    from mgadmm import _lib as lib
    blk = make_product(pc.meta(), "knn", compute_dtype=torch.float64)
    blk.max_ADMM_iter, blk.check_stop = 3, False
    _expect_refused(blk, pc.inputs().double(), lib, "float64")
    blk.close()


def test_per_sample_form_refused_for_a_graph_beyond_the_lds_path(env):
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
    _expect_refused(blk, y, lib, "cannot hold this graph", param_schedule={"mu_u": np.array([[1.0, 2.0], [2.0, 3.0]])})
    x = blk.solve(y, param_schedule={"mu_u": np.array([1.0, 2.0])})[0]      # the shared form runs there
    assert torch.isfinite(x).all()
    blk.close()


def test_per_sample_form_refused_with_the_whole_batch_stop_test(env):
    blk, lib = _blk("knn", "None")
    blk.check_stop, blk.ADMM_tol, blk.max_ADMM_iter = True, 1e-6, 5
    assert blk.admm_convergence == "whole_batch"
    _expect_refused(blk, pc.inputs(), lib, "whole_batch")
    blk.close()


def test_wrong_batch_and_a_name_given_twice_through_the_c_abi(env):
    import ctypes as C
    blk, lib = _blk("knn", "None")
    y = pc.inputs()
    blk.max_ADMM_iter = 3
    x_plain = blk.solve(y)[0]                                    # the solver exists, max_batch = 8
    h = _handle(blk)
    setp, sets = lib.lib.mgadmm_solver_set_param_schedule, lib.lib.mgadmm_solver_set_sample_params
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    err = lambda: lib.lib.mgadmm_last_error().decode()
    four = np.ones((5, 4)) * float(blk.mu_u)
    assert setp(h, C.byref(lib.ParamSchedule(mu_u=dp(four))), 5, 4, 0) == lib.OK
    blk._reset_history()
    with pytest.raises(lib.MgadmmError) as e:
        blk.solve(y)                                             # B = 8 against a table of 4 columns
    assert e.value.code == lib.ERR_INVALID and "param_schedule" in str(e.value) and "4 samples" in str(e.value) and blk.p_res_list == []
    assert setp(h, None, 0, 0, 0) == lib.OK
    assert torch.equal(blk.solve(y)[0], x_plain)
    # invalid tables
    nine = np.ones((2, 9))
    assert setp(h, C.byref(lib.ParamSchedule(rho=dp(nine))), 2, 9, 0) == lib.ERR_INVALID and "max_batch" in err()
    bad = np.ones((5, 8)); bad[3, 6] = 0.0
    assert setp(h, C.byref(lib.ParamSchedule(rho_u=dp(bad))), 5, 8, 0) == lib.ERR_INVALID and "rho_u[3][6]" in err()
    bad = np.ones(5); bad[2] = np.nan
    assert setp(h, C.byref(lib.ParamSchedule(mu_d1=dp(bad))), 5, 0, 0) == lib.ERR_INVALID and "mu_d1[2]" in err()
    assert setp(h, C.byref(lib.ParamSchedule(mu_d1=dp(np.ones(5)))), 5, 0, -1) == lib.ERR_INVALID and "first_row" in err()
    # a name given twice, in either order
    ones8, sched = np.ones(8) * float(blk.mu_u), np.ones((5, 8)) * float(blk.mu_u)
    assert sets(h, C.byref(lib.SampleParams(mu_u=dp(ones8))), 8) == lib.OK
    assert setp(h, C.byref(lib.ParamSchedule(mu_u=dp(sched))), 5, 8, 0) == lib.ERR_INVALID and "given twice" in err() and "mu_u" in err()
    assert sets(h, None, 0) == lib.OK
    assert setp(h, C.byref(lib.ParamSchedule(mu_u=dp(sched))), 5, 8, 0) == lib.OK
    assert sets(h, C.byref(lib.SampleParams(mu_u=dp(ones8))), 8) == lib.ERR_INVALID and "given twice" in err()
    assert sets(h, C.byref(lib.SampleParams(rho=dp(np.ones(8) * float(blk.rho)))), 8) == lib.OK      # another name: fine
    assert torch.equal(blk.solve(y)[0], x_plain)                 # both tables hold the scalars
    assert setp(h, None, 0, 0, 0) == lib.OK and sets(h, None, 0) == lib.OK
    # through Python the refusal of the library leaves no table behind
    with pytest.raises(ValueError, match="given twice"):
        blk.solve(y, sample_params={"mu_u": ones8}, param_schedule={"mu_u": sched})
    assert torch.equal(blk.solve(y)[0], x_plain)
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 11
def test_sweep_returns_the_grid_of_chains(env):
    from mgadmm.ADMM import geometric_ramp
    mode, abl = CASES[0]
    blk, lib = _blk(mode, abl)
    y = pc.inputs()[:2]
    inf = pc.info()
    ramps = [geometric_ramp(float(inf["rho"]), f, pc.N_ROWS) for f in (1.0, 1.1)]
    mus = [float(inf["mu_d1"]), 2 * float(inf["mu_d1"])]
    x, n, sets = blk.sweep(y, {"mu_d1": mus}, schedules={"rho": ramps})
    assert _unit(lib, blk) == 2
    assert tuple(x.shape) == (4, 2, 24, 30, 1) and n.shape == (4, 2) and (n == K).all()
    assert [s["mu_d1"] for s in sets] == [mus[0], mus[0], mus[1], mus[1]]
    assert all(np.array_equal(s["rho"], ramps[j % 2]) for j, s in enumerate(sets))
    one_blk, _ = _blk(mode, abl)
    for p in range(4):
        for w in range(2):
            one_blk.mu_d1 = float(sets[p]["mu_d1"])
            chain = _chain(one_blk, y[w:w + 1], abl, lambda it, p=p: {"rho": float(sets[p]["rho"][min(it, pc.N_ROWS - 1)])}, K)
            assert torch.equal(x[p, w], chain["x"][0]), (p, w)
    assert not torch.equal(x[0], x[1])                           # the two ramps differ
    blk.close(); one_blk.close()
