"""Buffers of a live solver that grow or are replaced between calls (csrc/dev_buf.h: every block and its capacity in one owner).
The 30-node kNN graph of g4_meta.npz (helpers.make_product), T = 24, t_in = 12: a float32 instance, whose solves take the
LDS-resident path, and a float64 instance on the streaming path.  Every result is compared with torch.equal, and every history
list element by element, against a fresh instance created with the final settings (the per-sample tables: against the B = 1
solves of instances that carry each sample's table as their own).

  1  iteration limits raised on a live solver (max_CG_iter 5 -> 40, max_ADMM_iter 2 -> 6): the CG scalars' history, the pinned
     log of active counts and the three ADMM history buffers grow; with and without record_cg_coeffs
  2  two_loops with max_inner_iter = 3 after a solve: its outer x inner rows outgrow the CG-count history; a solve follows
  3  a solver created for 70 samples solves 3, then 70: the partials of the streaming path grow with the batch, the LDS path
     adds the iterate buffers of a six-iteration chunk; workspace_bytes() after every step as the parent commit reported it
  4  a band table set for 5 samples, replaced by one for 3, then cleared, a solve after each (the lifetime of one table, also
     through the C ABI: test_gpu_band_sets.py::test_lifetime_of_the_table)
  5  graph tables set twice with other sigmas, then cleared, a solve after each (one table, then none:
     test_gpu_graph_sets.py::test_batch_of_8_with_4_sigma_pairs)
  6  apply_op_Ln twice on one instance: the second call reads the row sums the first one uploaded

No test makes an allocation or a copy fail: those paths are replayed on the CPU (tests/test_dev_buf_cpu.py)."""
import numpy as np
import pytest
import torch

import band_sets_cases as bc
import graph_sets_cases as gc
from conftest import load_golden
from helpers import make_product
from test_gpu_band_sets import _assert_sample_equals, _band_kw
from test_gpu_graph_sets import _assert_equals_solves_run_alone as _assert_equals_sigma_twins
from test_gpu_sample_params import _solve

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
INSTANCES = [("lds", F32), ("stream", F64)]
IDS = ["lds-float32", "stream-float64"]
LISTS = ("p_res_list", "d_res_list", "x_shift_list", "delta_x_per_step", "DGTV_list", "DGLR_list", "GLR_list", "recover_list",
         "CG_iter_x", "CG_iter_zu", "CG_iter_zd", "alpha_x", "beta_x", "alpha_zu", "beta_zu", "alpha_zd", "beta_zd")
# workspace_bytes() of the parent commit's library for the steps of test 3 (created for 70 samples; after the solve of 3;
# after the solve of 70), recorded once with that build: profiles/r21/README.txt
PARENT_WORKSPACE = {"lds-float32": (7741440, 9216000, 9216000), "stream-float64": (15482880, 21774336, 21774336)}


def _make(path, dtype, n_admm, n_cg, record=False, **kw):
    blk = make_product(load_golden("g4_meta.npz"), "knn", compute_dtype=dtype, path=path, record_cg_coeffs=record, **kw)
    blk.max_ADMM_iter, blk.max_CG_iter, blk.check_stop = n_admm, n_cg, False
    return blk


def _inputs(B, dtype, seed=21):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(100 + 50 * rng.random((B, 12, 30, 1))).to(dtype)


def _run(blk, y, call="solve"):
    """One solve (or two_loops) from a cleared history: x, the state and every history list."""
    blk._reset_history()
    x = blk.solve(y)[0] if call == "solve" else blk.two_loops(y)
    return dict(x=blk.state["x"] if x is None else x, state={k: v.clone() for k, v in blk.state.items()},
                lists={nm: [np.asarray(v).copy() for v in getattr(blk, nm)] for nm in LISTS})


def _assert_same(got, want, what):
    assert torch.isfinite(want["x"]).all(), what
    assert torch.equal(got["x"], want["x"]), (what, "x")
    assert set(got["state"]) == set(want["state"]), what
    for k, v in want["state"].items():
        assert torch.equal(got["state"][k], v), (what, "state", k)
    for nm in LISTS:
        a, b = got["lists"][nm], want["lists"][nm]
        assert len(a) == len(b), (what, nm, len(a), len(b))
        for i, (u, v) in enumerate(zip(a, b)):
            assert u.shape == v.shape and np.array_equal(u, v, equal_nan=True), (what, nm, i)


# ---------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("record", [False, True], ids=["plain", "record"])
@pytest.mark.parametrize("path, dtype", INSTANCES, ids=IDS)
def test_iteration_limits_raised_on_a_live_solver(path, dtype, record):
    y = _inputs(4, dtype)
    blk = _make(path, dtype, 2, 5, record)
    small = _run(blk, y)
    assert len(small["lists"]["p_res_list"]) == 2 and max(int(np.max(c)) for c in small["lists"]["CG_iter_x"]) <= 5
    blk.max_CG_iter, blk.max_ADMM_iter = 40, 6
    got = _run(blk, y)
    blk.close()
    fresh = _make(path, dtype, 6, 40, record)
    want = _run(fresh, y)
    fresh.close()
    # the raised limits are in use: six iterations, CG solves longer than the five the buffers were created for
    assert len(want["lists"]["p_res_list"]) == 6 and max(int(np.max(c)) for c in want["lists"]["CG_iter_x"]) > 5
    assert (len(want["lists"]["alpha_x"]) == 6) == record
    _assert_same(got, want, (path, record))


# ---------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("path, dtype", INSTANCES, ids=IDS)
def test_two_loops_outgrows_the_history_of_a_solve(path, dtype):
    y = _inputs(4, dtype)

    def two_loops_settings(blk):
        blk.max_ADMM_iter, blk.max_inner_iter = 2, 3          # 6 rows of CG counts, the solver was created for 2

    blk = _make(path, dtype, 2, 40)
    _run(blk, y)
    two_loops_settings(blk)
    loops = _run(blk, y, "two_loops")
    blk.max_ADMM_iter = 4
    last = _run(blk, y)
    blk.close()
    assert len(loops["lists"]["CG_iter_x"]) == 6 and len(last["lists"]["p_res_list"]) == 4

    fresh = _make(path, dtype, 2, 40)
    two_loops_settings(fresh)
    _assert_same(loops, _run(fresh, y, "two_loops"), (path, "two_loops"))
    fresh.close()
    fresh = _make(path, dtype, 4, 40)
    want = _run(fresh, y)
    fresh.close()
    _assert_same(last, want, (path, "the solve after two_loops"))


# ---------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("path, dtype", INSTANCES, ids=IDS)
def test_small_batch_then_the_full_batch_of_a_solver_created_for_70(path, dtype):
    from mgadmm import _lib
    tag = IDS[INSTANCES.index((path, dtype))]
    y = _inputs(70, dtype)
    blk = _make(path, dtype, 6, 40)          # (six iterations in one launch on the LDS path: more iterate buffers than the workspace lends)
    blk._solver(1, dtype, 70)
    ws = [blk.workspace_bytes(1, dtype)]
    _run(blk, y[:3])
    ws.append(blk.workspace_bytes(1, dtype))
    got = _run(blk, y)
    ws.append(blk.workspace_bytes(1, dtype))
    h = blk._solvers[(1, dtype)][0]
    assert _lib.lib.mgadmm_solver_path(h, 70) == (_lib.PATH_LDS if path == "lds" else _lib.PATH_STREAM)
    blk.close()
    print(f"\nworkspace_bytes {tag}: {ws}")
    assert tuple(ws) == PARENT_WORKSPACE[tag], (tag, ws)
    assert ws[0] < ws[-1]                     # (something was added after the creation: the ring buffers / the partials)
    fresh = _make(path, dtype, 6, 40)
    want = _run(fresh, y)
    assert fresh.workspace_bytes(1, dtype) == ws[-1]
    fresh.close()
    _assert_same(got, want, tag)


# ---------------------------------------------------------------------------------------------------------- 4
def test_band_table_replaced_for_another_batch_then_cleared():
    abl, n_it = "None", 3
    y, _ = bc.inputs(5)

    def prep(b):
        b.max_ADMM_iter, b.check_stop, b.record_cg_coeffs = n_it, False, False
        return b

    blk = prep(bc.instance(abl, path="lds"))
    steps = [(5, _band_kw(5)), (3, _band_kw(3)), (5, {})]
    sets_of = [bc.set_of_sample(5), bc.set_of_sample(3), [bc.INTERVALS.index(bc.WIDTH)] * 5]      # (no table: the instance's own width)
    batches = [_solve(blk, y[:B], abl, **kw) for B, kw in steps]
    blk.close()
    assert sets_of[0][0] != sets_of[2][0] and not torch.equal(batches[0]["x"][0], batches[2]["x"][0])      # the table was read, then gone
    twins = {}
    for step, ((B, _), sos, batch) in enumerate(zip(steps, sets_of, batches)):
        assert batch["n_iters"] == n_it
        for b in range(B):
            j = int(sos[b])
            if j not in twins:
                twins[j] = prep(bc.twin(abl, j, path="lds"))
            _assert_sample_equals(batch, b, _solve(twins[j], y[b:b + 1], abl), 0, f"step {step}")
    for t in twins.values():
        t.close()


# ---------------------------------------------------------------------------------------------------------- 5
def test_graph_tables_set_twice_then_cleared():
    mode, abl, n_it = "knn", "None", 6
    y = gc.inputs()[:4]
    pairs = gc.pairs()

    def prep(b):
        b.max_ADMM_iter, b.check_stop, b.record_cg_coeffs = n_it, False, False

    blk = gc.instance(mode, abl, *pairs[1], path="lds")
    prep(blk)
    orders = [[0, 1, 2, 3], [3, 0, 1, 2], [1, 1, 1, 1]]                                            # the pair of every sample; last: the instance's own
    kws = [dict(graph_params={"u_sigma": [pairs[j][0] for j in o], "d_sigma": [pairs[j][1] for j in o]}) for o in orders[:2]] + [{}]
    batches = [_solve(blk, y, abl, **kw) for kw in kws]
    blk.close()
    assert not torch.equal(batches[0]["x"][0], batches[1]["x"][0]) and not torch.equal(batches[1]["x"][0], batches[2]["x"][0])
    for order, batch in zip(orders, batches):
        assert batch["n_iters"] == n_it
        _assert_equals_sigma_twins(mode, abl, batch, y, None, range(4), lambda b: pairs[order[b]], prepare=prep, what=str(order))


# ---------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("path, dtype", INSTANCES, ids=IDS)
def test_apply_op_Ln_twice_reads_the_cached_row_sums(path, dtype):
    blk = _make(path, dtype, 2, 40)
    x = _inputs(3, dtype, seed=5).repeat(1, 2, 1, 1)          # (3, T, N, 1)
    first = blk.apply_op_Ln(x)
    second = blk.apply_op_Ln(x)
    blk.close()
    assert torch.isfinite(first).all() and float(first.abs().max()) > 0 and torch.equal(first, second)
    fresh = _make(path, dtype, 2, 40)
    assert torch.equal(fresh.apply_op_Ln(x), first)
    fresh.close()
