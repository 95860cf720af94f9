"""Every shipped k_admm_lds_ps / k_admm_lds_pp instance against its k_admm_lds twin (tests/lds_census.py: one row per instance).

The library compiles the 45 instances three times (csrc/lds_launch.hip, lds_launch_ps.hip, lds_launch_pp.hip); the census
(test_gpu_lds_census.py) pins the first compilation to the float64 oracle.  Here every census row runs through the other two,
and every picked sample must equal the B = 1 solve of the first compilation bit for bit: the three are built from one source
and promise the same arithmetic in the same order, so any difference is a wrong register, address or barrier.

Inputs: the census's inputs of the row with sample b scaled by lc.unit_scales (0.5 + 1.5 b / (B - 1): the samples converge at
different iterations); picks = samples 0, B // 2, B - 1.  Unit 'pp': sample b carries the census weights times ROWS[b % 8] of
test_gpu_sample_params.py; unit 'ps': no table.  One product instance per row (MGADMM_LDS_CHUNK=4, record_cg_coeffs=False)
serves every step:
  a. twin, fixed count: for every pick a B = 1 solve of K = lc.unit_k(r) iterations by the instance carrying the pick's six
     scalars, no table, whole-batch mode -> Q_LDS_UNIT 0 and the row's instance; x, state, per-sample metrics, CG counts kept;
  b. 'pp' only: the batch with the table, K iterations in chunks of 4 -> Q_LDS_UNIT 2 and the row's instance; every pick equals
     its twin bit for bit; pick B - 1 against the float64 oracle built with its row at F32_X_TOL = 1e-5;
  c. ADMM_tol = lc.pick_admm_tol of the twins' deciding residuals (max over the ablation's primal and dual residuals, square
     roots of the per-sample metric sums in float64): the picker asserts that every pick first crosses in [2, K - 1], that
     the crossings differ, that two picks stop in different launches, and that no residual lies within 1 % of the tolerance;
  d. the batch with admm_convergence='per_sample' and the stop test at that tolerance (with the table for 'pp') -> Q_LDS_UNIT 1
     ('ps') or 2 ('pp') and the row's instance; against B = 1 twins under the same tolerance with the whole-batch device stop
     test (Q_LDS_UNIT 0, one iteration per launch): n_iters_per_sample, x, every state vector, the first n_b rows of the
     per-sample metrics and the CG counts bit for bit, and n_b = the picker's crossing.  Every other sample: finite, and
     1 <= n_b <= K.
"""
import time

import numpy as np
import pytest
import torch

import lds_census as lc
from test_gpu_lds_census import _info, _inputs, _oracle, _product, env  # noqa: F401  (env: the fixture that clears the switches)
from test_gpu_sample_params import F32_X_TOL, NAMES, ROWS

pytestmark = pytest.mark.gpu

CG_LISTS = ("CG_iter_x", "CG_iter_zu", "CG_iter_zd")


def _table(info, B):
    """sample_params of a batch of B: sample b uses the census weights times ROWS[b % 8] (float64 products)."""
    return {nm: np.array([info[nm] * ROWS[b % 8][j] for b in range(B)]) for j, nm in enumerate(NAMES)}


def _carry(blk, weights):
    for nm in NAMES:
        setattr(blk, nm, float(weights[nm]))


def _solve(blk, y, mask, **kw):
    blk._reset_history()
    x = blk.solve(torch.from_numpy(y), mask=None if mask is None else torch.from_numpy(mask), per_sample_history=True, **kw)[0]
    cg = [np.stack([np.asarray(v).reshape(-1) for v in getattr(blk, nm)]) for nm in CG_LISTS if getattr(blk, nm)]
    return dict(x=x.clone(), state={k: v.clone() for k, v in blk.state.items()}, mps=blk.metrics_per_sample.copy(), cg=cg,
                n=blk.n_iters_per_sample.copy(), n_iters=len(blk.p_res_list))


def _deciding_residuals(mps, abl):
    """(iters,) float64: the residual that decides the stop test of a B = 1 solve after each iteration."""
    from mgadmm import _lib as L
    ms = [L.M_PRI_ZU, L.M_DUAL_ZU]
    if abl in ("None", "DGLR"):
        ms += [L.M_PRI_PHI, L.M_DUAL_PHI]
    if abl != "DGLR":
        ms += [L.M_PRI_ZD, L.M_DUAL_ZD]
    return np.sqrt(mps[:, ms, 0].astype(np.float64)).max(1)


def _assert_pick_equals_twin(tag, abl, batch, b, one, nb):
    assert torch.equal(batch["x"][b], one["x"][0]), (tag, b, "x")
    assert set(batch["state"]) == set(one["state"]), tag
    for k in one["state"]:
        assert torch.equal(batch["state"][k][b], one["state"][k][0]), (tag, b, "state." + k)
    assert one["mps"].shape[0] == nb and np.array_equal(batch["mps"][:nb, :, b], one["mps"][:, :, 0]), (tag, b, "metrics_per_sample")
    assert len(batch["cg"]) == len(one["cg"]) == (2 if abl == "DGLR" else 3), tag
    for nm, cb, c1 in zip(CG_LISTS, batch["cg"], one["cg"]):
        assert c1.shape[0] == nb and np.array_equal(cb[:nb, b], c1[:, 0]), (tag, b, nm)


@pytest.mark.parametrize("unit", lc.UNITS)
@pytest.mark.parametrize("r", lc.CENSUS, ids=lc.row_id)
def test_unit_instance_against_its_twin(r, unit, env):
    from mgadmm import _lib
    t0 = time.time()
    for k, v in r["env"].items():
        env.setenv(k, v)
    env.setenv("MGADMM_LDS_CHUNK", str(lc.UNIT_CHUNK))
    B, K, abl = r["B"], lc.unit_k(r), r["abl"]
    picks = lc.unit_picks(r)
    info = _info(r["N"], r["T"])
    y, mask = _inputs(r)
    y = (y * lc.unit_scales(r).reshape(B, 1, 1, 1)).astype(np.float32)
    table = _table(info, B) if unit == "pp" else None
    weights = lambda b: info if table is None else {nm: table[nm][b] for nm in NAMES}
    one_of = lambda a, b: None if a is None else a[b:b + 1]
    tag = f"{r['expect']} {unit} N={r['N']} T={r['T']} t_in={r['t_in']} {r['kind']} {abl} {r['task']} B={B}"

    blk = _product(r, info, path="lds")
    blk.max_ADMM_iter = K
    h = blk._solver(1, torch.float32, B)[0]
    ran = lambda: (_lib.query(h, _lib.Q_LDS_UNIT), _lib.lds_instance(h))
    assert ran() == (-1, None), tag                                                   # no launch yet
    assert _lib.query(h, _lib.Q_LDS_CHUNK) == lc.UNIT_CHUNK, tag

    # a. the twins: B = 1 solves of k_admm_lds, K iterations
    blk.check_stop, blk.admm_convergence = False, "whole_batch"
    twins = []
    for b in picks:
        _carry(blk, weights(b))
        twins.append(_solve(blk, y[b:b + 1], one_of(mask, b)))
        assert ran() == (0, r["expect"]), (tag, b, ran())
        assert twins[-1]["n_iters"] == K, (tag, b)
    assert blk._solvers[(1, torch.float32)][0].value == h.value                        # one solver throughout
    _carry(blk, info)

    # b. k_admm_lds_pp, K iterations with launch boundaries inside
    if unit == "pp":
        fixed = _solve(blk, y, mask, sample_params=table)
        assert ran() == (2, r["expect"]), (tag, ran())
        assert fixed["n_iters"] == K and (fixed["n"] == K).all(), tag
        for b, one in zip(picks, twins):
            _assert_pick_equals_twin(tag, abl, fixed, b, one, K)
        b = picks[-1]
        o = _oracle(r, blk, {nm: float(table[nm][b]) for nm in NAMES})
        xo = o.combined_loop(y[b:b + 1].astype(np.float64), mask=one_of(mask, b), n_iters=K)
        err = float(np.linalg.norm(fixed["x"][b:b + 1].double().numpy() - xo) / np.linalg.norm(xo))
        print(f"\n[census-units] {tag}: sample {b} (weights x {ROWS[b % 8].tolist()}) against the float64 oracle: {err:.2e}")
        assert err < F32_X_TOL, (tag, "x against the oracle built with the sample's weights", err)

    # c. the tolerance at which the picks stop at different iterations, in different launches, none on a rounding decision
    res = np.stack([_deciding_residuals(t["mps"], abl) for t in twins])
    tol, n_first = lc.pick_admm_tol(res, K)
    print(f"\n[census-units] {tag}: ADMM_tol {tol!r}, first crossings {n_first}")

    # d. the unit under test, every sample stopping on its own residuals
    blk.check_stop, blk.admm_convergence, blk.ADMM_tol = True, "per_sample", tol
    batch = _solve(blk, y, mask, **({} if table is None else dict(sample_params=table)))
    assert ran() == (1 if unit == "ps" else 2, r["expect"]), (tag, ran())
    n = batch["n"]
    assert n.shape == (B,) and (n >= 1).all() and (n <= K).all(), (tag, n)
    assert torch.isfinite(batch["x"]).all() and all(torch.isfinite(v).all() for v in batch["state"].values()), tag
    blk.admm_convergence = "whole_batch"
    for b, nf in zip(picks, n_first):
        _carry(blk, weights(b))
        one = _solve(blk, y[b:b + 1], one_of(mask, b))
        assert ran() == (0, r["expect"]), (tag, b, ran())
        nb = one["n_iters"]
        assert int(n[b]) == nb == int(one["n"][0]) == nf, (tag, b, int(n[b]), nb, nf)
        _assert_pick_equals_twin(tag, abl, batch, b, one, nb)
    blk.close()
    print(f"[census-units] {tag}: n_b of the picks {[int(n[b]) for b in picks]}, of the batch {int(n.min())}..{int(n.max())}; {time.time() - t0:.1f} s")
