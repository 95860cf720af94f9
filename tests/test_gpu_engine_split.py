"""What a float64 solver does with the features only the LDS-resident float32 path implements.  The float32 solver is
csrc/lds_engine.h's LdsEngine, the float64 one the plain Engine<double> of csrc/engine.h: the setters' host halves, the
refusals of csrc/solve_gate.h and the queries are the base's and answer for float64 as they did when both were one class.
Through the C ABI on ONE float64 solver of the N = 30 kNN fixture of tests/adaptive_rho_cases.py, B = 8, 3 iterations, no
stop test; every message is one of the pairs of tests/golden/solve_gate_parent.json."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import adaptive_rho_cases as ac
from conftest import GOLDEN
from helpers import make_product

pytestmark = pytest.mark.gpu

B, N_IT = 8, 3
F64 = ": float64 arithmetic runs on the streaming path"


def test_float64_solver_refuses_the_float32_only_features_and_solves_as_before():
    from mgadmm import _lib
    from mgadmm.ADMM import _ptr, _stream_ptr
    with open(os.path.join(GOLDEN, "solve_gate_parent.json")) as f:
        pairs = json.load(f)["pairs"]

    def golden(who, feature):
        """the one float64 refusal among the golden pairs that starts with `who: feature `"""
        found = [m for rc, m in pairs if rc == _lib.ERR_UNSUPPORTED and m.startswith(f"{who}: {feature} ") and m.endswith(F64)]
        assert len(found) == 1, (who, feature, found)
        return found[0]

    blk = make_product(ac.meta(), "knn", ablation="None", compute_dtype=torch.float64)
    blk.max_ADMM_iter, blk.check_stop, blk.record_cg_coeffs = N_IT, False, False
    yd = blk._dev_tensor(ac.inputs(), torch.float64, "y", blk.t_in)
    assert yd.shape[0] == B and yd.shape[2] == 30
    h, _ = blk._solver(1, torch.float64, B)
    lib, f64p = _lib.lib, C.POINTER(C.c_double)

    def solve():
        """(rc, message, x, n_iters, metrics) of one mgadmm_solve; x and metrics start as NaN"""
        x = torch.full((B, blk.T, 30, 1), float("nan"), device=yd.device, dtype=torch.float64)
        metrics = np.full((N_IT, _lib.NMETRIC), np.nan)
        hs, st = _lib.History(), _lib.State()
        hs.metrics = metrics.ctypes.data_as(f64p)
        rc = lib.mgadmm_solve(h, _ptr(yd), None, 0, B, _ptr(x), C.byref(st), C.byref(hs), _stream_ptr(yd.device))
        torch.cuda.synchronize()
        return rc, lib.mgadmm_last_error().decode(), x.cpu().numpy(), hs.n_iters, metrics

    def refused(want):
        rc, msg, x, n, m = solve()
        assert rc == _lib.ERR_UNSUPPORTED and msg == want, (rc, msg)
        assert n == 0 and np.isnan(m).all() and np.isnan(x).all()      # nothing ran

    # (e) no LDS plan, the streaming path
    assert _lib.query(h, _lib.Q_LDS_OK) == 0 and lib.mgadmm_solver_path(h, B) == _lib.PATH_STREAM

    # (a) a plain solve
    rc, _, x_plain, n, m_plain = solve()
    assert rc == _lib.OK and n == N_IT and np.isfinite(x_plain).all() and np.isfinite(m_plain).all()

    # (b) the table is taken, the solve that would read it is refused
    rho = float(ac.info()["rho"]) * np.linspace(0.5, 2.0, B)
    table = _lib.SampleParams()
    table.rho = rho.ctypes.data_as(f64p)
    assert lib.mgadmm_solver_set_sample_params(h, C.byref(table), B) == _lib.OK
    refused(golden("solve", "sample_params"))

    # (c) adaptive penalties alone
    _lib.check(lib.mgadmm_solver_set_sample_params(h, None, 0))
    ar = _lib.AdaptiveRho(every=1, until=0, mu=1.25, tau=2.0)
    ar.rho_min[:], ar.rho_max[:] = [ac.RHO_MIN] * 3, [ac.RHO_MAX] * 3
    _lib.check(lib.mgadmm_solver_set_adaptive_rho(h, C.byref(ar), 0))
    refused(golden("solve", "adaptive_rho"))
    n_periods = C.c_int32(-1)
    _lib.check(lib.mgadmm_solver_get_adaptive_history(h, B, None, 0, C.byref(n_periods)))
    assert n_periods.value == 0
    _lib.check(lib.mgadmm_solver_set_adaptive_rho(h, None, 0))

    # (d) a graph table is refused when it is set, even one of the solver's own graph; clearing is always allowed
    handles = (C.c_void_p * 1)(blk._graph(1).handle)
    set_of = np.zeros(B, dtype=np.int32)
    rc = lib.mgadmm_solver_set_sample_graphs(h, 1, handles, set_of.ctypes.data_as(C.POINTER(C.c_int32)), B)
    assert rc == _lib.ERR_UNSUPPORTED and lib.mgadmm_last_error().decode() == golden("set_sample_graphs", "sample_graphs")
    assert lib.mgadmm_solver_set_sample_graphs(h, 0, None, None, 0) == _lib.OK

    # (e) again, (f) with everything cleared the plain solve of before, bit for bit
    assert _lib.query(h, _lib.Q_LDS_OK) == 0 and lib.mgadmm_solver_path(h, B) == _lib.PATH_STREAM
    rc, _, x, n, m = solve()
    assert rc == _lib.OK and n == N_IT
    assert np.array_equal(x, x_plain) and np.array_equal(m, m_plain)
    blk.close()
