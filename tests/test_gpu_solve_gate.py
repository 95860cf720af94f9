"""The library answers with the texts and in the order of csrc/solve_gate.h (tests/test_solve_gate_cpu.py checks the header
against the golden file on the CPU; this ties libmgadmm.so to it).  Through the C ABI on ONE solver of the N = 30 kNN
fixture of tests/adaptive_rho_cases.py, B = 8, 3 iterations, no stop test: a sample_params table, a per-sample
param_schedule and adaptive_rho are set together and the path is set to MGADMM_PATH_STREAM, so that three refusals are due.
The solve reports the first of the header's order and runs nothing; with adaptive_rho cleared, the next one; with
everything cleared, the plain solve of before, bit for bit."""
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

# copied from the distinct pairs of tests/golden/solve_gate_parent.json
ADAPTIVE = ("solve: adaptive_rho (penalties adapted on the device) is implemented by the LDS-resident float32 path only: "
            "path is MGADMM_PATH_STREAM")
SAMPLE = ("solve: sample_params (per-sample ADMM weights) are implemented by the LDS-resident float32 path only: "
          "path is MGADMM_PATH_STREAM")
B, N_IT = 8, 3


def test_the_first_refusal_due_is_reported_and_nothing_runs():
    from mgadmm import _lib
    from mgadmm.ADMM import _ptr, _stream_ptr
    with open(os.path.join(GOLDEN, "solve_gate_parent.json")) as f:
        pairs = json.load(f)["pairs"]
    assert [_lib.ERR_UNSUPPORTED, ADAPTIVE] in pairs and [_lib.ERR_UNSUPPORTED, SAMPLE] in pairs

    blk = make_product(ac.meta(), "knn", ablation="None", path="lds")
    blk.max_ADMM_iter, blk.check_stop, blk.record_cg_coeffs = N_IT, False, False
    yd = blk._dev_tensor(ac.inputs(), torch.float32, "y", blk.t_in)
    assert yd.shape[0] == B and yd.shape[2] == 30
    h, p = blk._solver(1, torch.float32, B)
    lib, f64p = _lib.lib, C.POINTER(C.c_double)

    def solve():
        """(rc, message, x, n_iters, metrics) of one mgadmm_solve; x and metrics start as NaN"""
        x = torch.full((B, blk.T, 30, 1), float("nan"), device=yd.device)
        metrics = np.full((N_IT, _lib.NMETRIC), np.nan)
        hs, st = _lib.History(), _lib.State()
        hs.metrics = metrics.ctypes.data_as(f64p)
        rc = lib.mgadmm_solve(h, _ptr(yd), None, 0, B, _ptr(x), C.byref(st), C.byref(hs), _stream_ptr(yd.device))
        torch.cuda.synchronize()
        return rc, lib.mgadmm_last_error().decode(), x.cpu().numpy(), hs.n_iters, metrics

    def set_path(path):
        p.path = path
        _lib.check(lib.mgadmm_solver_set_params(h, C.byref(p)))

    rc, _, x_plain, n, m_plain = solve()
    assert rc == _lib.OK and n == N_IT and np.isfinite(x_plain).all() and np.isfinite(m_plain).all()

    info = ac.info()
    rho = float(info["rho"]) * np.linspace(0.5, 2.0, B)
    rho_u = float(info["rho_u"]) * np.linspace(0.5, 2.0, 5 * B).reshape(5, B)
    table, sched = _lib.SampleParams(), _lib.ParamSchedule()
    table.rho, sched.rho_u = rho.ctypes.data_as(f64p), rho_u.ctypes.data_as(f64p)
    ar = _lib.AdaptiveRho(every=1, until=0, mu=1.25, tau=2.0)
    ar.rho_min[:], ar.rho_max[:] = [ac.RHO_MIN] * 3, [ac.RHO_MAX] * 3
    _lib.check(lib.mgadmm_solver_set_sample_params(h, C.byref(table), B))
    _lib.check(lib.mgadmm_solver_set_param_schedule(h, C.byref(sched), 5, B, 0))
    _lib.check(lib.mgadmm_solver_set_adaptive_rho(h, C.byref(ar), 0))
    set_path(_lib.PATH_STREAM)

    for clear, want in ((None, ADAPTIVE), (lambda: lib.mgadmm_solver_set_adaptive_rho(h, None, 0), SAMPLE)):
        if clear:
            _lib.check(clear())
        rc, msg, x, n, m = solve()
        assert rc == _lib.ERR_UNSUPPORTED and msg == want, (rc, msg)
        assert n == 0 and np.isnan(m).all() and np.isnan(x).all()      # nothing ran

    _lib.check(lib.mgadmm_solver_set_sample_params(h, None, 0))
    _lib.check(lib.mgadmm_solver_set_param_schedule(h, None, 0, 0, 0))
    set_path(_lib.PATH_LDS)
    rc, _, x, n, m = solve()
    assert rc == _lib.OK and n == N_IT
    assert np.array_equal(x, x_plain) and np.array_equal(m, m_plain)
    blk.close()
