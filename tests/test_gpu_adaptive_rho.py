"""Adaptive ADMM penalties on the LDS path (solve(adaptive_rho=..., adaptive_start=...), mgadmm_solver_set_adaptive_rho):
after every `every`-th iteration each sample balances rho_u, rho and rho_d on its own residual sums (csrc/lds_adapt.h), on
the device, between two launches of k_admm_lds_pp.  An adaptive solve equals, bit for bit, the CHAIN it replaces: B = 1
solves of `every` iterations by k_admm_lds with scalar penalties, resumed with warm_start=, the numpy rule of
tests/adaptive_rho_cases.py applied to the last row of metrics_per_sample between them; and lies within the project's
float32 tolerances of the float64 twin, whose decisions it must repeat exactly.

Fixture (tests/adaptive_rho_cases.py): tables of g4_meta.npz, the 8 inputs of g5_batched.npz, four cases, K = 20 iterations,
every = 4: five steps, the last one after the last iteration (what a resumed solve starts from)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import adaptive_rho_cases as ac
import graph_sets_cases as gc
import lds_census as lc
from helpers import check_windows, make_product, rel
from test_gpu_lds_census import _info as census_info, _inputs as census_inputs, _product as census_product, env  # noqa: F401
from test_gpu_lds_census_units import _deciding_residuals
from test_gpu_param_schedule import _assert_same, _assert_sample_equals, _handle, _unit
from test_gpu_sample_params import ROWS, _solve, _table

pytestmark = pytest.mark.gpu

NAMES, CASES, IDS, K = ac.NAMES, ac.CASES, ac.IDS, ac.K
CHAIN_TRIPLE = (4, 1.25, 4.0)      # chains read the very doubles the device reads: no margin is needed, any triple that steps will do


def _blk(mode, abl, n_it=K, **kw):
    from mgadmm import _lib
    kw.setdefault("path", "lds")
    blk = make_product(ac.meta(), mode, ablation=abl, **kw)
    blk.max_ADMM_iter, blk.check_stop = n_it, False
    blk.record_cg_coeffs = False              # the chunked schedule (several iterations per launch)
    return blk, _lib


def _asolve(blk, y, abl, triple=CHAIN_TRIPLE, until=None, ad=None, **kw):
    """An adaptive solve: the snapshot of test_gpu_sample_params._solve with rho_history (P, 3, B) and rho_final (3, B).
    ad: the adaptive_rho dict (default: `triple` with the wide clamps)."""
    out = _solve(blk, y, abl, adaptive_rho=ad or ac.adaptive_dict(*triple, until=until), **kw)
    out["rho_history"], out["rho_final"] = blk.rho_history.copy(), blk.rho_final.copy()
    return out


def _adaptive_chain(blk, y, abl, triple, n_it, start_w=None, until=None, mask=None):
    """The host-driven loop the feature replaces, for ONE sample: solves of at most `every` iterations by `blk` with the
    penalties assigned as the instance's scalars (no table of any kind: k_admm_lds), each resumed from the state of the one
    before; after a solve that ends on a step, ac.step on the last row of its metrics_per_sample.  start_w: the six start
    weights (default: the instance's).  Returns a snapshot like _solve with the rows of all iterations, and rho_history."""
    every, mu, tau = triple
    if not hasattr(blk, "_weights_as_built"):      # (an earlier chain left its last penalties on the instance)
        blk._weights_as_built = {nm: float(getattr(blk, nm)) for nm in NAMES}
    for nm, v in dict(blk._weights_as_built, **(start_w or {})).items():
        setattr(blk, nm, float(v))
    w = {nm: np.array([float(getattr(blk, nm))]) for nm in NAMES[:3]}
    hist = [[float(w[nm][0]) for nm in NAMES[:3]]]
    state, segs, it = None, [], 0
    while it < n_it:
        n = min(every - it % every, n_it - it)
        blk.max_ADMM_iter, blk.check_stop = n, False
        for nm in NAMES[:3]:
            setattr(blk, nm, float(w[nm][0]))
        segs.append(_solve(blk, y, abl, warm_start=state, mask=mask))
        assert segs[-1]["n_iters"] == n
        state, it = segs[-1]["state"], it + n
        if ac.steps_after(it - 1, 0, every, until):
            w = ac.step(w, segs[-1]["mps"][-1], abl, mu, tau)
            hist.append([float(w[nm][0]) for nm in NAMES[:3]])
    out = dict(segs[-1])
    out["mps"] = np.concatenate([s["mps"] for s in segs])
    out["cg"] = [np.concatenate([s["cg"][k] for s in segs]) for k in range(len(segs[0]["cg"]))]
    out["n_iters"], out["rho_history"] = it, np.array(hist)
    return out


def _assert_history(batch, b, hist, what=""):
    got = batch["rho_history"][:, :, b]
    assert got.shape == hist.shape and np.array_equal(got, hist), (what, b, got.tolist(), hist.tolist())
    assert np.array_equal(batch["rho_final"][:, b], hist[-1]), (what, b)


@functools.lru_cache(maxsize=None)
def _batch(i):
    """The adaptive batch of 8 of case i with CHAIN_TRIPLE, default launch shape (asserted: launches of 4, k_admm_lds_pp)."""
    mode, abl = CASES[i]
    blk, lib = _blk(mode, abl)
    out = _asolve(blk, ac.inputs(), abl)
    assert lib.query(_handle(blk), lib.Q_LDS_CHUNK) > 4 and _unit(lib, blk) == 2
    assert out["n_iters"] == K and (out["n"] == K).all() and out["rho_history"].shape == (6, 3, 8)
    blk.close()
    return out


@functools.lru_cache(maxsize=None)
def _chains(i):
    mode, abl = CASES[i]
    one_blk, lib = _blk(mode, abl)
    y = ac.inputs()
    out = [_adaptive_chain(one_blk, y[b:b + 1], abl, CHAIN_TRIPLE, K) for b in range(8)]
    assert _unit(lib, one_blk) == 0
    one_blk.close()
    return out


# ---------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_adaptive_batch_equals_the_chain_bit_for_bit(i, env):
    batch, chains = _batch(i), _chains(i)
    moved = 0
    for b in range(8):
        _assert_sample_equals(batch, b, chains[b], IDS[i])
        _assert_history(batch, b, chains[b]["rho_history"], IDS[i])
        moved += int((chains[b]["rho_history"][1:] != chains[b]["rho_history"][:-1]).sum())
    print(IDS[i], "penalty changes over the 8 chains:", moved)
    assert moved >= 8          # the penalties move: the comparison is not one of constant-penalty solves


# ---------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_every_sample_matches_its_float64_twin(i, env):
    """The project's own tolerances: 1e-5 on x, 1e-3 on the history, +-1 on the CG counts; the history of the penalties
    exactly (the twin's decisions lie >= 1 % from their thresholds: tests/test_lds_adapt_cpu.py).

    The penalties are clamped as tests/adaptive_rho_cases.py reasons: without clamps they fall to 1/16 of the fixture's values,
    where a float32 CG count lies 2 ... 8 iterations from the float64 one in plain constant-penalty solves too (measured on one
    MI355X with the unclamped triples: x to 4e-7, residuals to 1e-3, rho_history exact, but an x solve of line-None 3 and a zu
    solve of physical-DGTV 2 iterations off)."""
    mode, abl = CASES[i]
    triple = ac.triple(i)
    blk, _ = _blk(mode, abl)
    blk._reset_history()
    x = blk.solve(ac.inputs(), per_sample_history=True, adaptive_rho=ac.twin_dict(i, *triple))[0]
    twins = ac.twin_solutions(i, *triple)
    for b in range(8):
        xo, o = twins[b]
        print("sample", b, "rel x against the twin", rel(x[b:b + 1], xo))
        assert np.array_equal(blk.rho_history[:, :, b], ac.twin_history(o)), (b, blk.rho_history[:, :, b].tolist(), ac.twin_history(o).tolist())
        check_windows(f"{IDS[i]} sample {b}", blk, x, [b], o, xo, xtol=ac.F32_X_TOL, htol=ac.F32_HIST_RTOL, slack=1, abl=abl)
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 3
def _assert_same_adaptive(a, b, what):
    _assert_same(a, b, what)
    assert np.array_equal(a["rho_history"], b["rho_history"]) and np.array_equal(a["rho_final"], b["rho_final"]), what


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_other_launch_shapes_give_the_same_bits(i, env):
    mode, abl = CASES[i]
    ref = _batch(i)                           # (the default launch shape: before the switches below)
    for chunk in ("2", "1"):
        env.setenv("MGADMM_LDS_CHUNK", chunk)
        blk, lib = _blk(mode, abl)
        got = _asolve(blk, ac.inputs(), abl)
        assert lib.query(_handle(blk), lib.Q_LDS_CHUNK) == int(chunk) and _unit(lib, blk) == 2
        _assert_same_adaptive(got, ref, "launches of " + chunk)
        blk.close()
    env.delenv("MGADMM_LDS_CHUNK")
    env.setenv("MGADMM_LDS_ASYNC", "0")       # the synchronous schedule: one iteration per launch, one stream
    blk, lib = _blk(mode, abl)
    sync = _asolve(blk, ac.inputs(), abl)
    assert _unit(lib, blk) == 2
    _assert_same_adaptive(sync, ref, "synchronous schedule")
    blk.close()


@pytest.mark.parametrize("every", [16, 1])
def test_a_period_of_16_and_of_1(every, env):
    """every = 16 with 20 iterations: launches of 16 + 4, one step; every = 1: a step after every iteration, launches of one."""
    mode, abl = CASES[0]
    triple = (every,) + CHAIN_TRIPLE[1:]
    blk, lib = _blk(mode, abl)
    batch = _asolve(blk, ac.inputs(), abl, triple=triple)
    assert _unit(lib, blk) == 2 and batch["rho_history"].shape[0] == 1 + K // every
    one_blk, _ = _blk(mode, abl)
    for b in (0, 5):
        chain = _adaptive_chain(one_blk, ac.inputs()[b:b + 1], abl, triple, K)
        _assert_sample_equals(batch, b, chain, f"every {every}")
        _assert_history(batch, b, chain["rho_history"], f"every {every}")
        assert (chain["rho_history"][-1] != chain["rho_history"][0]).any()
    blk.close(); one_blk.close()


# ---------------------------------------------------------------------------------------------------------- 4
def _alone(one_blk, y, abl, b, start_w=None, **kw):
    for nm, v in (start_w or {}).items():
        setattr(one_blk, nm, float(v))
    return _asolve(one_blk, y[b:b + 1], abl, **kw)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_batch_of_8_equals_eight_adaptive_solves_run_alone(i, env):
    mode, abl = CASES[i]
    batch = _batch(i)
    one_blk, lib = _blk(mode, abl)
    for b in range(8):
        one = _alone(one_blk, ac.inputs(), abl, b)
        _assert_sample_equals(batch, b, one, IDS[i])
        _assert_history(batch, b, one["rho_history"][:, :, 0], IDS[i])
    assert _unit(lib, one_blk) == 2
    one_blk.close()


def test_start_values_per_sample(env):
    """The per-sample table (ROWS of test_gpu_sample_params.py) gives the start values; the mus of a row never change."""
    mode, abl = CASES[0]
    table, y = _table(), ac.inputs()
    blk, lib = _blk(mode, abl)
    batch = _asolve(blk, y, abl, sample_params=table)
    assert _unit(lib, blk) == 2
    assert np.array_equal(batch["rho_history"][0], np.stack([table[nm] for nm in NAMES[:3]]))
    one_blk, _ = _blk(mode, abl)
    for b in range(8):
        row = {nm: table[nm][b] for nm in NAMES}
        one_blk.max_ADMM_iter = K                 # (a chain leaves the length of its last solve behind)
        _assert_sample_equals(batch, b, _alone(one_blk, y, abl, b, row), "start values")
        if b in (3, 7):
            chain = _adaptive_chain(one_blk, y[b:b + 1], abl, CHAIN_TRIPLE, K, start_w=row)
            _assert_sample_equals(batch, b, chain, "start values, chain")
            _assert_history(batch, b, chain["rho_history"], "start values, chain")
    blk.close(); one_blk.close()


def test_with_graph_params(env):
    """Samples 2j, 2j + 1 on the graph of sigma pair j (test_gpu_graph_sets.py), every one with its own adaptation."""
    mode, abl = CASES[0]
    pairs, sos, y = gc.pairs(), np.repeat(np.arange(4), 2), ac.inputs()
    gp = {"u_sigma": [pairs[j][0] for j in sos], "d_sigma": [pairs[j][1] for j in sos]}
    blk = gc.instance(mode, abl, *pairs[1], path="lds")
    blk.max_ADMM_iter, blk.check_stop, blk.record_cg_coeffs = K, False, False
    batch = _asolve(blk, y, abl, graph_params=gp)
    differ = 0
    for b in (0, 3, 6):
        one_blk = gc.instance(mode, abl, *pairs[sos[b]], path="lds")
        one_blk.max_ADMM_iter, one_blk.check_stop, one_blk.record_cg_coeffs = K, False, False
        one = _alone(one_blk, y, abl, b)
        _assert_sample_equals(batch, b, one, "graph_params")
        _assert_history(batch, b, one["rho_history"][:, :, 0], "graph_params")
        one_blk.close()
    for b in range(0, 8, 2):
        differ += not np.array_equal(batch["rho_history"][:, :, 0], batch["rho_history"][:, :, b])
    print("samples whose penalties differ from sample 0's:", differ)
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 5
def test_per_sample_stopping(env):
    """ADMM_tol by lc.pick_admm_tol on the deciding residuals of the adaptive twins (no residual within 1 % of it): the
    samples stop at different iterations, in different launches of 4; past its stop a sample's history is NaN."""
    i = 0
    mode, abl = CASES[i]
    triple = ac.triple(i)
    every = triple[0]
    res = []
    for _, o in ac.twin_solutions(i, *triple):
        res.append([max(max(p), max(d)) for p, d in zip(o.hist.p_res_list, o.hist.d_res_list)])
    tol, n_first = lc.pick_admm_tol(np.array(res), K, chunk=every)
    print("\nADMM_tol", tol, "first crossings", n_first)
    blk, lib = _blk(mode, abl, admm_convergence="per_sample")
    blk.ADMM_tol, blk.check_stop = tol, True
    batch = _asolve(blk, ac.inputs(), abl, ad=ac.twin_dict(i, *triple))
    assert _unit(lib, blk) == 2 and batch["n"].tolist() == n_first and batch["n_iters"] == max(n_first)
    one_blk, _ = _blk(mode, abl, admm_convergence="per_sample")
    one_blk.ADMM_tol, one_blk.check_stop = tol, True
    for b in range(8):
        nb = n_first[b]
        one = _alone(one_blk, ac.inputs(), abl, b, ad=ac.twin_dict(i, *triple))
        assert one["n_iters"] == nb
        assert torch.equal(batch["x"][b], one["x"][0]), b
        for k in one["state"]:
            assert torch.equal(batch["state"][k][b], one["state"][k][0]), (b, k)
        assert np.array_equal(batch["mps"][:nb, :, b], one["mps"][:nb, :, 0]), b
        rows = 1 + (nb - 1) // every          # the start values and the steps the sample was still running at
        hb = batch["rho_history"][:, :, b]
        assert np.isfinite(hb[:rows]).all() and np.isnan(hb[rows:]).all(), (b, nb, hb.tolist())
        assert np.array_equal(hb[:rows], one["rho_history"][:rows, :, 0]) and np.array_equal(batch["rho_final"][:, b], hb[rows - 1]), b
    assert len(set(n_first)) > 1
    blk.close(); one_blk.close()


# ---------------------------------------------------------------------------------------------------------- 6
def test_resume(env):
    mode, abl = CASES[0]
    full, y = _batch(0), ac.inputs()
    blk, lib = _blk(mode, abl, n_it=8)
    first = _asolve(blk, y, abl)
    assert first["rho_history"].shape[0] == 3 and np.array_equal(first["rho_history"], full["rho_history"][:3])
    blk.max_ADMM_iter = K - 8
    start = {nm: first["rho_final"][f] for f, nm in enumerate(NAMES[:3])}
    second = _asolve(blk, y, abl, sample_params=start, adaptive_start=8, warm_start=first["state"])
    assert second["n_iters"] == K - 8
    for k in ("x", "zu", "zd", "phi"):
        assert torch.equal(second[k], full[k]), k
    for k in full["state"]:
        assert torch.equal(second["state"][k], full["state"][k]), k
    assert np.array_equal(np.concatenate([first["mps"], second["mps"]]), full["mps"])
    assert np.array_equal(np.concatenate([first["rho_history"][:-1], second["rho_history"]]), full["rho_history"])
    assert np.array_equal(second["rho_final"], full["rho_final"])
    with pytest.raises(ValueError, match="adaptive_start = 6"):
        blk.solve(y, adaptive_rho=ac.adaptive_dict(*CHAIN_TRIPLE), adaptive_start=6, warm_start=first["state"])
    ar = lib.AdaptiveRho(every=4, until=0, mu=2.0, tau=2.0)
    ar.rho_min[:], ar.rho_max[:] = [1e-6] * 3, [1e6] * 3
    assert lib.lib.mgadmm_solver_set_adaptive_rho(_handle(blk), C.byref(ar), 6) == lib.ERR_INVALID
    msg = lib.lib.mgadmm_last_error().decode()
    assert "adaptive_rho" in msg and "start = 6" in msg, msg
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 7
def test_until_8(env):
    mode, abl = CASES[0]
    blk, lib = _blk(mode, abl)
    batch = _asolve(blk, ac.inputs(), abl, until=8)
    assert batch["rho_history"].shape[0] == 3 and np.array_equal(batch["rho_history"], _batch(0)["rho_history"][:3])
    one_blk, _ = _blk(mode, abl)
    for b in (1, 6):
        chain = _adaptive_chain(one_blk, ac.inputs()[b:b + 1], abl, CHAIN_TRIPLE, K, until=8)
        assert chain["rho_history"].shape[0] == 3
        _assert_sample_equals(batch, b, chain, "until 8")
        _assert_history(batch, b, chain["rho_history"], "until 8")
    assert not torch.equal(batch["x"], _batch(0)["x"])
    blk.close(); one_blk.close()


# ---------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_a_rule_that_never_steps_is_the_plain_solve(i, env):
    mode, abl = CASES[i]
    blk, lib = _blk(mode, abl)
    plain = _solve(blk, ac.inputs(), abl)
    assert _unit(lib, blk) == 0
    inst = lib.lds_instance(_handle(blk))
    never = _asolve(blk, ac.inputs(), abl, triple=(4, 1e30, 2.0))
    assert _unit(lib, blk) == 2 and lib.lds_instance(_handle(blk)) == inst
    _assert_same(never, plain, "mu = 1e30")
    start = [float(ac.info()[nm]) for nm in NAMES[:3]]
    assert never["rho_history"].shape == (6, 3, 8) and (never["rho_history"] == np.array(start)[None, :, None]).all()
    after = _solve(blk, ac.inputs(), abl)                              # cleared after the call
    assert _unit(lib, blk) == 0 and blk.rho_history is None
    _assert_same(after, plain, "after")
    assert not torch.equal(_batch(i)["x"], plain["x"])
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 9
def test_more_samples_than_compute_units(env):
    """B = 1024 = 128 start sets x 8 windows (window index fastest): set j starts from the fixture's penalties times
    0.5 + 1.5 j / 127; 12 iterations."""
    mode, abl = CASES[0]
    P, W, n_it = 128, 8, 12
    scale = np.repeat(0.5 + 1.5 * np.arange(P) / (P - 1), W)
    table = {nm: float(ac.info()[nm]) * scale for nm in NAMES[:3]}
    y = ac.inputs().repeat(P, 1, 1, 1)
    blk, lib = _blk(mode, abl, n_it=n_it)
    batch = _asolve(blk, y, abl, sample_params=table)
    assert _unit(lib, blk) == 2 and batch["n_iters"] == n_it and batch["rho_history"].shape == (4, 3, P * W)
    one_blk, _ = _blk(mode, abl, n_it=n_it)
    for b in (0, 517, 1023):
        one = _alone(one_blk, y, abl, b, {nm: table[nm][b] for nm in NAMES[:3]})
        _assert_sample_equals(batch, b, one, "B = 1024")
        _assert_history(batch, b, one["rho_history"][:, :, 0], "B = 1024")
    blk.close(); one_blk.close()


# ---------------------------------------------------------------------------------------------------------- 10
CENSUS_ROWS = [lc.uni(8, 1024, True, 2), lc.uni(8, 1024, True, -1), lc.inst(3, False, 1024, False), lc.inst(12, False, 640, True),
               lc.inst(2, True, 1024, False)]
CENSUS_K, CENSUS_B = 12, 6


@pytest.mark.parametrize("expect", CENSUS_ROWS, ids=[lc.row_id(dict(expect=e)) for e in CENSUS_ROWS])
def test_census_rows(expect, env):
    """Uniform rows with a compile-time tail (TP 2), uniform rows with a run-time tail, a generic instance with ragged rows, a
    single-buffer instance and a band instance: B = 6, every = 4, 12 iterations; sample b starts from the penalties times
    0.5 + 0.3 b.  Three samples against their chains."""
    from mgadmm import _lib
    r = dict(next(r for r in lc.CENSUS if r["expect"] == expect), B=CENSUS_B)
    for k, v in r["env"].items():
        env.setenv(k, v)
    abl, info = r["abl"], census_info(r["N"], r["T"])
    y, mask = census_inputs(r)
    yt, mt = torch.from_numpy(y), None if mask is None else torch.from_numpy(mask)
    table = {nm: float(info[nm]) * (0.5 + 0.3 * np.arange(CENSUS_B)) for nm in NAMES[:3]}
    blk = census_product(r, info, path="lds")
    blk.max_ADMM_iter, blk.check_stop = CENSUS_K, False
    batch = _asolve(blk, yt, abl, mask=mt, sample_params=table)
    h = _handle(blk)
    assert (_lib.query(h, _lib.Q_LDS_UNIT), _lib.lds_instance(h)) == (2, expect)
    assert batch["n_iters"] == CENSUS_K and batch["rho_history"].shape == (4, 3, CENSUS_B)
    one_blk = census_product(r, info, path="lds")
    for b in (0, 3, 5):
        chain = _adaptive_chain(one_blk, yt[b:b + 1], abl, CHAIN_TRIPLE, CENSUS_K, start_w={nm: table[nm][b] for nm in NAMES[:3]},
                                mask=None if mt is None else mt[b:b + 1])
        ht = _handle(one_blk)
        assert (_lib.query(ht, _lib.Q_LDS_UNIT), _lib.lds_instance(ht)) == (0, expect), b
        _assert_sample_equals(batch, b, chain, "census")
        _assert_history(batch, b, chain["rho_history"], "census")
    blk.close(); one_blk.close()


# ---------------------------------------------------------------------------------------------------------- 11
def _expect_refused(blk, y, lib, reason, code=None, **kw):
    blk._reset_history()
    kw.setdefault("adaptive_rho", ac.adaptive_dict(*CHAIN_TRIPLE))
    with pytest.raises(lib.MgadmmError) as e:
        blk.solve(y, **kw)
    assert e.value.code == (lib.ERR_UNSUPPORTED if code is None else code), e.value
    assert "adaptive_rho" in str(e.value) and reason in str(e.value), e.value
    assert blk.p_res_list == [] and blk.rho_history is None      # nothing ran
    x = blk.solve(y)[0]                                          # the same instance still solves normally
    assert torch.isfinite(x).all() and len(blk.p_res_list) > 0


def test_refused_on_the_streaming_path(env):
    blk, lib = _blk("knn", "None", n_it=3, path="stream")
    _expect_refused(blk, ac.inputs(), lib, "MGADMM_PATH_STREAM")
    blk.close()


def test_refused_in_float64(env):
    from mgadmm import _lib as lib
    blk = make_product(ac.meta(), "knn", compute_dtype=torch.float64)
    blk.max_ADMM_iter, blk.check_stop = 3, False
    _expect_refused(blk, ac.inputs().double(), lib, "float64")
    blk.close()


def test_refused_with_batch_max_cg_convergence(env):
    blk, lib = _blk("knn", "None", n_it=3, path="auto", cg_convergence="batch_max")
    _expect_refused(blk, ac.inputs(), lib, "batch_max")
    blk.close()


def test_refused_for_a_graph_beyond_the_lds_path(env):
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
    _expect_refused(blk, y, lib, "cannot hold this graph")
    blk.close()


def test_refused_with_the_whole_batch_stop_test(env):
    blk, lib = _blk("knn", "None", n_it=5)
    blk.check_stop, blk.ADMM_tol = True, 1e-6
    assert blk.admm_convergence == "whole_batch"
    _expect_refused(blk, ac.inputs(), lib, "whole_batch")
    blk.close()


def test_a_schedule_and_another_batch_through_the_c_abi(env):
    blk, lib = _blk("knn", "None", n_it=3)
    y = ac.inputs()
    x_plain = blk.solve(y)[0]                                    # the solver exists, max_batch = 8
    h = _handle(blk)
    seta, setp, sets = (lib.lib.mgadmm_solver_set_adaptive_rho, lib.lib.mgadmm_solver_set_param_schedule,
                        lib.lib.mgadmm_solver_set_sample_params)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    err = lambda: lib.lib.mgadmm_last_error().decode()
    ar = lib.AdaptiveRho(every=4, until=0, mu=2.0, tau=2.0)
    ar.rho_min[:], ar.rho_max[:] = [1e-6] * 3, [1e6] * 3
    # a param schedule set at the same time
    sched = np.ones(5) * float(blk.mu_u)
    assert setp(h, C.byref(lib.ParamSchedule(mu_u=dp(sched))), 5, 0, 0) == lib.OK and seta(h, C.byref(ar), 0) == lib.OK
    blk._reset_history()
    with pytest.raises(lib.MgadmmError) as e:
        blk.solve(y)
    assert e.value.code == lib.ERR_UNSUPPORTED and "adaptive_rho" in str(e.value) and "param_schedule" in str(e.value) and blk.p_res_list == []
    assert setp(h, None, 0, 0, 0) == lib.OK
    # a per-sample table of another batch size
    four = np.ones(4) * float(blk.rho)
    assert sets(h, C.byref(lib.SampleParams(rho=dp(four))), 4) == lib.OK
    with pytest.raises(lib.MgadmmError) as e:
        blk.solve(y)
    assert e.value.code == lib.ERR_INVALID and "adaptive_rho" in str(e.value) and "4 samples" in str(e.value) and blk.p_res_list == []
    assert sets(h, None, 0) == lib.OK
    # invalid parameters, by name
    for field, value, word in (("every", 0, "every = 0"), ("every", 17, "every = 17"), ("mu", 1.0, "mu = 1"), ("tau", 0.5, "tau = 0.5"),
                               ("until", -2, "until = -2")):
        bad = lib.AdaptiveRho(every=4, until=0, mu=2.0, tau=2.0)
        bad.rho_min[:], bad.rho_max[:] = [1e-6] * 3, [1e6] * 3
        setattr(bad, field, value)
        assert seta(h, C.byref(bad), 0) == lib.ERR_INVALID and "adaptive_rho" in err() and word in err(), err()
    bad = lib.AdaptiveRho(every=4, until=0, mu=2.0, tau=2.0)
    bad.rho_min[:], bad.rho_max[:] = [1e-6, 2.0, 1e-6], [1e6, 1.0, 1e6]
    assert seta(h, C.byref(bad), 0) == lib.ERR_INVALID and "rho_min[rho_u]" in err()
    # the setting that was accepted is still in force; cleared, the solver solves as before
    n = C.c_int32(-1)
    blk.solve(y)
    assert lib.lib.mgadmm_solver_get_adaptive_history(h, 8, None, 0, C.byref(n)) == lib.OK and n.value == 1      # 3 iterations: no step
    assert seta(h, None, 0) == lib.OK
    assert torch.equal(blk.solve(y)[0], x_plain)
    assert lib.lib.mgadmm_solver_get_adaptive_history(h, 8, None, 0, C.byref(n)) == lib.OK and n.value == 0
    blk.close()


def test_sweep_passes_adaptive_rho_through(env):
    mode, abl = CASES[0]
    blk, lib = _blk(mode, abl)
    y = ac.inputs()[:2]
    rhos = [float(ac.info()["rho"]), 2 * float(ac.info()["rho"])]
    x, n, sets = blk.sweep(y, {"rho": rhos}, adaptive_rho=ac.adaptive_dict(*CHAIN_TRIPLE))
    assert _unit(lib, blk) == 2 and tuple(x.shape) == (2, 2, 24, 30, 1) and (n == K).all()
    assert blk.rho_history.shape == (6, 3, 4) and np.array_equal(blk.rho_history[0, 0], np.repeat(rhos, 2))
    one_blk, _ = _blk(mode, abl)
    for p in range(2):
        for w in range(2):
            chain = _adaptive_chain(one_blk, y[w:w + 1], abl, CHAIN_TRIPLE, K, start_w={"rho": rhos[p]})
            assert torch.equal(x[p, w], chain["x"][0]), (p, w)
            assert np.array_equal(blk.rho_history[:, :, p * 2 + w], chain["rho_history"]), (p, w)
    blk.close(); one_blk.close()
