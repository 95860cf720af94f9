"""What solve() sets on a solver for one call does not outlive the call, whichever of the four arguments it was and also when
the library refuses the solve inside the scope (mgadmm/solve_args.py: solve_scope).  The kNN graph of
tests/golden/g1_tables_small.npz as tests/test_lds_graph_sets_cpu.py builds it, T = 24, t_in = 12, B = 3, 4 iterations, float32,
the LDS path.  With check_stop and the whole-batch stop test csrc/solve_gate.h refuses a solve with sample_params,
graph_params, a per-sample param_schedule or adaptive_rho; afterwards, with check_stop off, the plain solve of the same
instance equals a fresh instance's bit for bit and ran k_admm_lds, the kernel of a solver with no table set."""
import numpy as np
import pytest
import torch

from test_lds_graph_sets_cpu import _knn

pytestmark = pytest.mark.gpu

B, N_IT = 3, 4
ARGS = {
    "sample_params": dict(sample_params={"rho": [0.5, 1.0, 2.0]}),
    "graph_params": dict(graph_params={"u_sigma": [5.0, 10.0, 5.0]}),
    "param_schedule": dict(param_schedule={"rho_u": np.linspace(0.5, 2.0, 2 * B).reshape(2, B)}),
    "adaptive_rho": dict(adaptive_rho={"every": 2}),
}


def _blk():
    blk = _knn(path="lds")
    assert (blk.T, blk.t_in, blk.compute_dtype) == (24, 12, torch.float32)
    blk.max_ADMM_iter, blk.check_stop = N_IT, False
    return blk


def _plain(blk, y):
    from mgadmm import _lib
    blk._reset_history()
    x, (zu, zd), phi, _ = blk.solve(y)
    unit = _lib.LDS_UNITS[_lib.query(blk._solvers[(1, torch.float32)][0], _lib.Q_LDS_UNIT)]
    return dict(x=x, zu=zu, zd=zd, phi=phi), np.array(blk.p_res_list + blk.d_res_list), unit


@pytest.fixture(scope="module")
def fresh():
    blk = _blk()
    y = 100 + 50 * torch.from_numpy(np.random.default_rng(16).random((B, 12, blk.n_nodes, 1))).float()
    out = (y,) + _plain(blk, y)
    blk.close()
    return out


@pytest.mark.parametrize("name", list(ARGS))
def test_nothing_stays_set_after_a_solve_the_library_refused(fresh, name):
    from mgadmm import _lib
    y, want, want_res, unit = fresh
    assert unit == "k_admm_lds" and all(torch.isfinite(t).all() for t in want.values()) and want_res.shape == (2 * N_IT, 3)
    blk = _blk()
    blk.check_stop = True
    assert blk.admm_convergence == "whole_batch"
    with pytest.raises(_lib.MgadmmError) as e:
        blk.solve(y, **ARGS[name])
    assert e.value.code == _lib.ERR_UNSUPPORTED and blk.p_res_list == [], e.value          # refused, nothing ran
    blk.check_stop = False
    got, res, unit = _plain(blk, y)
    assert unit == "k_admm_lds"
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert np.array_equal(res, want_res)
    blk.close()
