"""Per-sample stopping of the outer ADMM loop (admm_convergence='per_sample'): every sample of a batch stops on its own
residuals, so that B samples are B independent B = 1 runs -- bit for bit against the B = 1 solves of the product, within one
iteration against the float64 oracle run on every sample alone.

All cases: tables of g4_meta.npz, the 8 inputs y of g5_batched.npz, prediction task, float32, path='lds',
max_ADMM_iter = 150, and the tolerances at which the oracle's stop iterations are the ones of TABLE."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import make_oracle, make_product, rel

pytestmark = pytest.mark.gpu

F32_X_TOL = 1e-5          # the agreement test_gpu_parity.py demands of float32 solves against the float64 oracle
F32_HIST_RTOL = 1e-3
MAX_IT = 150
# (mode, ablation, ADMM_tol, oracle stop iteration of every sample solved alone, oracle whole-batch stop iteration)
TABLE = [
    ("knn", "None", 7.348, [42, 58, 66, 61, 59, 65, 70, 62], 133),
    ("knn", "DGLR", 10.36, [42, 64, 62, 58, 60, 61, 69, 65], 125),
    ("line", "None", 7.193, [40, 59, 64, 58, 55, 65, 68, 65], 124),
    ("physical", "DGTV", 6.433, [36, 49, 67, 58, 56, 68, 70, 65], 142),
]
IDS = [f"{m}-{a}" for m, a, *_ in TABLE]


def _meta():
    return load_golden("g4_meta.npz")


def _y():
    return torch.from_numpy(load_golden("g5_batched.npz")["y"].astype(np.float32))


def _blk(mode, abl, tol, **kw):
    from mgadmm import _lib
    blk = make_product(_meta(), mode, ablation=abl, path="lds", **kw)
    blk.max_ADMM_iter, blk.ADMM_tol = MAX_IT, tol
    blk.record_cg_coeffs = False              # the chunked schedule (several iterations per launch)
    return blk, _lib


def _has(abl):
    return abl in ("None", "DGLR"), abl != "DGLR"


def _snapshot(blk, x, zs, phi, abl):
    """What a solve left behind, detached from the instance (the history lists are reset between solves)."""
    has_phi, has_zd = _has(abl)
    cg = [torch.stack([torch.as_tensor(v).reshape(-1) for v in getattr(blk, nm)]).numpy()
          for nm in ("CG_iter_x", "CG_iter_zu") + ("CG_iter_zd",) * has_zd]
    return dict(x=x.clone(), zu=zs[0].clone(), zd=zs[1].clone(), phi=None if phi is None else phi.clone(),
                n=blk.n_iters_per_sample.copy(), mps=blk.metrics_per_sample.copy(), cg=cg, n_iters=len(blk.p_res_list),
                pri=np.array(blk.p_res_list), dual=np.array(blk.d_res_list), dxps=list(blk.delta_x_per_step),
                state={k: v.clone() for k, v in blk.state.items()})


def _solve(blk, y, abl, **kw):
    blk._reset_history()
    x, zs, phi, _ = blk.solve(y, per_sample_history=True, **kw)
    return _snapshot(blk, x, zs, phi, abl)


def _assert_equals_single_runs(blk, lib, y, mask, abl, batch, samples):
    """Every sample of `samples` of the per-sample batch result against today's B = 1 solve of it (whole_batch mode).
    Zero tolerance: one workgroup owns one sample, runs the same instruction stream on it whatever the batch around it is,
    and takes the stop decision from the same doubles with the same comparisons."""
    blk.admm_convergence = "whole_batch"
    for b in samples:
        one = _solve(blk, y[b:b + 1], abl, mask=None if mask is None else mask[b:b + 1])
        nb = one["n_iters"]
        assert int(batch["n"][b]) == nb == int(one["n"][0]), (b, batch["n"][b], nb)
        for k in ("x", "zu", "zd", "phi"):
            if one[k] is not None:
                assert torch.equal(batch[k][b], one[k][0]), (b, k)
        assert np.array_equal(batch["mps"][:nb, :, b], one["mps"][:, :, 0]), b
        for cb, c1 in zip(batch["cg"], one["cg"]):
            assert np.array_equal(cb[:nb, b], c1[:, 0]), b
    blk.admm_convergence = "per_sample"


@functools.lru_cache(maxsize=None)
def _oracle_runs(i):
    """The oracle alone on every sample with the stop test: (n_b, x after n_b iterations, history of that run)."""
    mode, abl, tol, _, _ = TABLE[i]
    y = _y().double().numpy()
    out = []
    for b in range(y.shape[0]):
        o = make_oracle(_meta(), mode, ablation=abl)
        o.ADMM_tol, o.max_ADMM_iter = tol, MAX_IT
        xo = o.combined_loop(y[b:b + 1])
        out.append((len(o.hist.p_res_list), xo, o.hist))
    return out


@functools.lru_cache(maxsize=None)
def _batch_solve(i):
    mode, abl, tol, _, _ = TABLE[i]
    blk, lib = _blk(mode, abl, tol, admm_convergence="per_sample")
    h = blk._solver(1, torch.float32, 8)[0]
    assert lib.query(h, lib.Q_LDS_CHUNK) > 1
    s = _solve(blk, _y(), abl)
    blk.close()
    return s


# ---------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("i", range(len(TABLE)), ids=IDS)
def test_batch_equals_single_sample_solves_bit_for_bit(i):
    mode, abl, tol, _, _ = TABLE[i]
    blk, lib = _blk(mode, abl, tol, admm_convergence="per_sample")
    h = blk._solver(1, torch.float32, 8)[0]
    assert lib.query(h, lib.Q_LDS_CHUNK) > 1
    y = _y()
    batch = _solve(blk, y, abl)
    print("n_iters_per_sample", batch["n"].tolist())
    assert batch["n"].dtype == np.int32 and batch["n"].shape == (8,)
    _assert_equals_single_runs(blk, lib, y, None, abl, batch, range(8))
    blk.close()


def test_interpolation_batch_equals_single_sample_solves_bit_for_bit():
    """Interpolation task with a float32 mask.  g5_batched.npz holds prediction inputs only: its solved x serves as the full
    series, y = x * mask.  The tolerance is chosen as for TABLE: the median over the samples of the oracle's largest residual
    at iteration 61 of a run without stop test; if the stop iterations then span fewer than 10 iterations the samples are
    scaled by 1 + b / 4 first."""
    meta = _meta()
    xs = load_golden("g5_batched.npz")["x"].astype(np.float64)
    mask64 = np.broadcast_to(meta["mask"].astype(np.float64), xs.shape).copy()

    def pick(xfull):
        y64 = xfull * mask64
        worst = []
        for b in range(8):
            o = make_oracle(meta, "knn")
            o.ADMM_tol = 0.0
            o.combined_loop(y64[b:b + 1], mask=mask64[b:b + 1], n_iters=62)
            worst.append([max(max(p), max(d)) for p, d in zip(o.hist.p_res_list, o.hist.d_res_list)])
        worst = np.array(worst)                              # (8, 62)
        tol = float(np.median(worst[:, 61]))
        stops = []
        for b in range(8):
            o = make_oracle(meta, "knn")
            o.ADMM_tol, o.max_ADMM_iter = tol, MAX_IT
            o.combined_loop(y64[b:b + 1], mask=mask64[b:b + 1])
            stops.append(len(o.hist.p_res_list))
        return y64, tol, stops

    y64, tol, stops = pick(xs)
    if max(stops) - min(stops) < 10:
        y64, tol, stops = pick(xs * (1 + np.arange(8) / 4).reshape(8, 1, 1, 1))
    print("interpolation: ADMM_tol", tol, "oracle stops", stops)
    assert max(stops) - min(stops) >= 10, stops
    blk, lib = _blk("knn", "None", tol, admm_convergence="per_sample")
    y, mask = torch.from_numpy(y64.astype(np.float32)), torch.from_numpy(mask64.astype(np.float32))
    batch = _solve(blk, y, "None", mask=mask)
    print("n_iters_per_sample", batch["n"].tolist())
    _assert_equals_single_runs(blk, lib, y, mask, "None", batch, range(8))
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("i", range(len(TABLE)), ids=IDS)
def test_stop_iterations_and_iterates_match_the_oracle(i):
    """|n_b - n_b(oracle)| <= 1: in all four cases the oracle's deciding residual falls monotonically from iteration 5 on, by
    a factor >= 1.012 per iteration near the stop, and F32_HIST_RTOL = 1e-3 is the agreement demanded of float32 history
    entries -- the crossing of the tolerance can move by one iteration at most."""
    mode, abl, tol, table_n, _ = TABLE[i]
    has_phi, has_zd = _has(abl)
    runs = _oracle_runs(i)
    n_orc = np.array([r[0] for r in runs])
    assert np.abs(n_orc - np.array(table_n)).max() <= 1 and n_orc.max() - n_orc.min() >= 20, n_orc      # the fixture discriminates
    s = _batch_solve(i)
    print("n_b", s["n"].tolist(), "oracle", n_orc.tolist())
    assert np.abs(s["n"] - n_orc).max() <= 1, (s["n"], n_orc)
    from mgadmm import _lib as L
    y = _y().double().numpy()
    res = [(L.M_PRI_ZU, L.M_DUAL_ZU)] + [(L.M_PRI_PHI, L.M_DUAL_PHI)] * has_phi + [(L.M_PRI_ZD, L.M_DUAL_ZD)] * has_zd
    for b in range(8):
        nb = int(s["n"][b])
        o = make_oracle(_meta(), mode, ablation=abl)
        xo = o.combined_loop(y[b:b + 1], n_iters=nb)               # exactly n_b iterations, no stop test
        assert len(o.hist.p_res_list) == nb
        err = rel(s["x"][b:b + 1], xo)
        print("sample", b, "n_b", nb, "rel x", err)
        assert err < F32_X_TOL, (b, err)
        floor = 1e-7 * float(np.linalg.norm(xo))
        mps = s["mps"][:nb, :, b]
        pri = np.sqrt(np.stack([mps[:, p] for p, _ in res], 1))
        dual = np.sqrt(np.stack([mps[:, d] for _, d in res], 1))
        np.testing.assert_allclose(pri, np.array(o.hist.p_res_list), rtol=F32_HIST_RTOL, atol=floor, err_msg=f"primal {b}")
        np.testing.assert_allclose(dual, np.array(o.hist.d_res_list), rtol=F32_HIST_RTOL, atol=floor, err_msg=f"dual {b}")


# ---------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("i", range(len(TABLE)), ids=IDS)
def test_history_of_a_per_sample_solve(i):
    mode, abl, tol, _, _ = TABLE[i]
    has_phi, has_zd = _has(abl)
    from mgadmm import _lib as L
    s = _batch_solve(i)
    n, mps = s["n"].astype(np.int64), s["mps"]
    nit = s["n_iters"]
    assert nit == n.max() and mps.shape == (nit, L.NMETRIC, 8)
    for b in range(8):
        assert np.isfinite(mps[:n[b], :, b]).all() and np.isnan(mps[n[b]:, :, b]).all(), b
        for c in s["cg"]:
            assert (c[:n[b], b] > 0).all() and (c[n[b]:, b] == 0).all(), b
    assert s["dxps"] == []
    # whole-batch rows = the per-sample rows with a stopped sample standing still: its difference terms are 0, its other
    # terms stay at their last values (the same doubles in another order of summation: rtol 1e-12)
    diff = (L.M_XSHIFT, L.M_DUAL_ZU, L.M_DUAL_PHI, L.M_DUAL_ZD)
    frozen = np.empty_like(mps)
    for b in range(8):
        frozen[:n[b], :, b] = mps[:n[b], :, b]
        frozen[n[b]:, :, b] = mps[n[b] - 1, :, b]
        for m in diff:
            frozen[n[b]:, m, b] = 0.0
    norm = np.sqrt(frozen.sum(2))                                # (iters, NMETRIC)
    res = [(L.M_PRI_ZU, L.M_DUAL_ZU)] + [(L.M_PRI_PHI, L.M_DUAL_PHI)] * has_phi + [(L.M_PRI_ZD, L.M_DUAL_ZD)] * has_zd
    np.testing.assert_allclose(s["pri"], np.stack([norm[:, p] for p, _ in res], 1), rtol=1e-12)
    np.testing.assert_allclose(s["dual"], np.stack([norm[:, d] for _, d in res], 1), rtol=1e-12)
    # the other lists, through a solve of their own (the snapshot keeps the residual lists only)
    blk, _ = _blk(mode, abl, tol, admm_convergence="per_sample")
    blk.solve(_y(), per_sample_history=True)
    assert np.array_equal(blk.metrics_per_sample, mps, equal_nan=True)
    np.testing.assert_allclose(np.array(blk.x_shift_list), norm[:, L.M_XSHIFT], rtol=1e-12)
    np.testing.assert_allclose(np.array(blk.recover_list), norm[:, L.M_RECOVER], rtol=1e-12)
    np.testing.assert_allclose(torch.stack(blk.GLR_list).numpy(), frozen[:, L.M_GLR].mean(1), rtol=1e-12)
    if has_phi:
        np.testing.assert_allclose(torch.stack(blk.DGTV_list).numpy(), frozen[:, L.M_DGTV].mean(1), rtol=1e-12)
    if has_zd:
        np.testing.assert_allclose(torch.stack(blk.DGLR_list).numpy(), frozen[:, L.M_DGLR].mean(1), rtol=1e-12)
    assert blk.delta_x_per_step == [] and blk.history()["n_iters_per_sample"] is blk.n_iters_per_sample
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("i", range(len(TABLE)), ids=IDS)
def test_off_means_off(i):
    mode, abl, tol, _, n_whole = TABLE[i]
    blk, lib = _blk(mode, abl, tol)
    assert blk.admm_convergence == "whole_batch"
    y = _y()
    w = _solve(blk, y, abl)
    print("whole-batch n_iters", w["n_iters"], "oracle", n_whole)
    assert abs(w["n_iters"] - n_whole) <= 1                      # same argument as for the per-sample counts
    assert (w["n"] == w["n_iters"]).all() and len(w["dxps"]) == w["n_iters"]
    # without the stop test the mode is a fixed-count solve
    blk.check_stop = False
    blk.max_ADMM_iter = 40
    fixed = _solve(blk, y, abl)
    blk.admm_convergence = "per_sample"
    ps = _solve(blk, y, abl)
    assert ps["n_iters"] == fixed["n_iters"] == 40 and (ps["n"] == 40).all() and (fixed["n"] == 40).all()
    for k in ("x", "zu", "zd", "phi"):
        if fixed[k] is not None:
            assert torch.equal(ps[k], fixed[k]), k
    for k in fixed["state"]:
        assert torch.equal(ps["state"][k], fixed["state"][k]), k
    assert np.array_equal(ps["mps"], fixed["mps"]) and np.array_equal(ps["pri"], fixed["pri"])
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("i", range(len(TABLE)), ids=IDS)
def test_resume_in_per_sample_mode(i):
    """k1 = 30 fixed iterations, then a warm start with the stop test: iteration counting starts at 0 in the second call, so a
    sample stops there at n_b - 30 with the x of the one-call solve (the bit-for-bit resume property of mgadmm_solve_from)."""
    mode, abl, tol, _, _ = TABLE[i]
    k1 = 30
    full = _batch_solve(i)
    assert (full["n"] > k1).all()
    blk, _ = _blk(mode, abl, tol, admm_convergence="per_sample")
    y = _y()
    blk.check_stop, blk.max_ADMM_iter = False, k1
    first = _solve(blk, y, abl)
    assert (first["n"] == k1).all()
    blk.check_stop, blk.max_ADMM_iter = True, MAX_IT - k1
    second = _solve(blk, y, abl, warm_start=first["state"])
    print("resumed n_b", second["n"].tolist())
    assert np.array_equal(second["n"], full["n"] - k1)
    assert torch.equal(second["x"], full["x"])
    for k in ("zu", "zd", "phi"):
        if full[k] is not None:
            assert torch.equal(second[k], full[k]), k
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 6
def _expect_unsupported(blk, y, lib):
    with pytest.raises(lib.MgadmmError) as e:
        blk.solve(y)
    assert e.value.code == lib.ERR_UNSUPPORTED, e.value
    assert "per_sample" in str(e.value)
    assert blk.p_res_list == []                                  # nothing ran
    blk.admm_convergence = "whole_batch"                         # the same instance still solves in the default mode
    x = blk.solve(y)[0]
    assert torch.isfinite(x).all() and len(blk.p_res_list) == blk.max_ADMM_iter


def test_refused_on_the_streaming_path():
    blk, lib = _blk("knn", "None", 7.348, admm_convergence="per_sample")
    blk.path, blk.max_ADMM_iter, blk.check_stop = "stream", 3, False
    _expect_unsupported(blk, _y(), lib)
    blk.close()


def test_refused_by_set_params_on_a_live_solver():
    """The solver exists (whole_batch solve first), then the mode arrives through set_params together with the streaming path."""
    blk, lib = _blk("knn", "None", 7.348)
    blk.max_ADMM_iter, blk.check_stop = 3, False
    y = _y()
    blk.solve(y)
    blk._reset_history()
    blk.admm_convergence, blk.path = "per_sample", "stream"
    _expect_unsupported(blk, y, lib)
    blk.close()


def test_refused_in_float64():
    from mgadmm import _lib as lib
    blk = make_product(_meta(), "knn", compute_dtype=torch.float64, admm_convergence="per_sample")
    blk.max_ADMM_iter, blk.check_stop = 3, False
    _expect_unsupported(blk, _y().double(), lib)
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
                         tables=(torch.from_numpy(cl), torch.from_numpy(dl)), admm_convergence="per_sample")
    blk.max_ADMM_iter, blk.check_stop = 3, False
    y = torch.from_numpy((1 + rng.random((2, 12, N, 1))).astype(np.float32))
    _expect_unsupported(blk, y, lib)
    blk.close()


def test_bad_enum_value_is_invalid():
    """Any other value of the field -> MGADMM_ERR_INVALID from solver_create and from set_params."""
    import ctypes as C
    blk, lib = _blk("knn", "None", 7.348)
    h, p = blk._solver(1, torch.float32, 8)
    p.admm_convergence = 2
    assert lib.lib.mgadmm_solver_set_params(h, C.byref(p)) == lib.ERR_INVALID
    h2 = C.c_void_p()
    assert lib.lib.mgadmm_solver_create(blk._graph(1).handle, C.byref(p), 8, C.byref(h2)) == lib.ERR_INVALID
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 7
def test_more_samples_than_compute_units():
    """B = 1024: several rounds of workgroups per CU, samples stop in different launches.  The 8 inputs tiled, sample b scaled
    by 1 + (b // 8) / 128; 16 samples spread over the batch against their B = 1 solves."""
    mode, abl, tol, _, _ = TABLE[0]
    B = 1024
    y = _y().repeat(B // 8, 1, 1, 1) * (1 + (torch.arange(B) // 8).float() / 128).reshape(B, 1, 1, 1)
    blk, lib = _blk(mode, abl, tol, admm_convergence="per_sample")
    batch = _solve(blk, y, abl)
    n = batch["n"]
    print("B = 1024: n_b min / median / max", n.min(), int(np.median(n)), n.max(), "sum", int(n.sum()))
    assert batch["n_iters"] == n.max() and n.max() - n.min() >= 20
    picks = [(j * 67 + 5) % B for j in range(16)]
    assert len({p % 8 for p in picks}) == 8 and len(set(picks)) == 16
    _assert_equals_single_runs(blk, lib, y, None, abl, batch, picks)
    blk.close()


# ---------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("i", [0, 3], ids=[IDS[0], IDS[3]])
def test_recording_cg_coefficients_takes_one_iteration_per_launch_with_the_same_result(i):
    """record_cg_coeffs switches to the synchronous schedule (one iteration per launch, the host reads the count of stopped
    samples after each): same n_b, x, state and per-sample history as the chunked schedule; alpha / beta of a sample are NaN
    past its last iteration."""
    mode, abl, tol, _, _ = TABLE[i]
    has_phi, has_zd = _has(abl)
    full = _batch_solve(i)
    blk, _ = _blk(mode, abl, tol, admm_convergence="per_sample")
    blk.record_cg_coeffs = True
    s = _solve(blk, _y(), abl)
    assert np.array_equal(s["n"], full["n"]) and s["n_iters"] == full["n_iters"]
    for k in ("x", "zu", "zd", "phi"):
        if full[k] is not None:
            assert torch.equal(s[k], full[k]), k
    assert np.array_equal(s["mps"], full["mps"], equal_nan=True) and np.array_equal(s["pri"], full["pri"])
    for a, b in zip(s["cg"], full["cg"]):
        assert np.array_equal(a, b)
    for w, (al, be) in enumerate(((blk.alpha_x, blk.beta_x), (blk.alpha_zu, blk.beta_zu)) + (((blk.alpha_zd, blk.beta_zd),) * has_zd)):
        al, be = torch.stack(al).numpy(), torch.stack(be).numpy()          # (iters, max_CG_iter, B)
        assert al.shape[0] == s["n_iters"]
        for b in range(8):
            nb = int(s["n"][b])
            assert np.isnan(al[nb:, :, b]).all() and np.isnan(be[nb:, :, b]).all(), (w, b)
            for it in range(nb):
                k = int(s["cg"][w][it, b])
                assert np.isfinite(al[it, :k, b]).all() and np.isnan(al[it, k:, b]).all(), (w, b, it)
    blk.close()
