"""CPU checks of per-iteration ADMM weights (mgadmm_solver_set_param_schedule, solve(param_schedule=..., schedule_start=...),
sweep(schedules=...), geometric_ramp).  None of it needs a GPU.

  * tests/cpu/lds_param_table_check.cpp (AddressSanitizer + UBSan, a program of its own) on csrc/lds_param_table.h: clamping
    and first_row, the fallbacks schedule -> per-sample table -> scalar, a one-row schedule giving the records the engine
    formed before schedules existed byte for byte, the refusals by name;
  * the header's declaration, the ctypes mirror, the exported symbol, the launch arguments;
  * validation in Python before the library is touched;
  * sweep(schedules=) forming the product, and passing nothing new without schedules;
  * geometric_ramp;
  * the float64 twin of tests/param_schedule_cases.py discriminates: its solution under the schedule differs from the
    constant-weight solution and from the schedule shifted by one row by the margins the GPU tests rely on."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import param_schedule_cases as pc             # noqa: E402
from helpers import _tiny, rel                # noqa: E402

NAMES = list(pc.NAMES)


# ------------------------------------------------------------------------------------------------ the header's own check
def test_table_builder_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "lds_param_table_check")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpu", "lds_param_table_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    res = json.loads(out.stdout)
    assert res["record_bytes"] == 32
    assert res["refusals"] == ["t: rho_d[2][3] is not finite", "t: rho_d[3][4] is not finite", "t: rho_d[1][0] = 0, should be > 0",
                               "t: mu_d2[0][2] = -0.5, should be >= 0", "t: rho_u[3] = -1, should be > 0", "mu_d1"]


def test_the_header_is_plain_cxx():
    txt = open(os.path.join(PKG, "csrc", "lds_param_table.h")).read()
    assert "hip" not in re.sub(r"//.*", "", txt).lower() and "getenv" not in txt


# ------------------------------------------------------------------------------------------------ ABI
def test_header_binding_and_symbol_agree():
    from mgadmm import _lib
    raw = open(os.path.join(ROOT, "include", "mgadmm.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"typedef struct \{([^{}]*)\} mgadmm_param_schedule;", txt)
    assert m and re.findall(r"\*(\w+)", m.group(1)) == NAMES and "const double" in m.group(1)
    assert re.search(r"int mgadmm_solver_set_param_schedule\(mgadmm_solver\* s, const mgadmm_param_schedule\* sch, int32_t n_rows, "
                     r"int32_t B,\s*int32_t first_row\);", txt)
    res, args = _lib.SYMBOLS["mgadmm_solver_set_param_schedule"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(_lib.ParamSchedule), C.c_int32, C.c_int32, C.c_int32]
    assert [f[0] for f in _lib.ParamSchedule._fields_] == NAMES and C.sizeof(_lib.ParamSchedule) == 6 * C.sizeof(C.c_void_p)
    assert _lib.lib.mgadmm_solver_set_param_schedule.argtypes == args
    assert _lib.lib.mgadmm_solver_set_param_schedule(None, None, 0, 0, 0) == _lib.ERR_INVALID
    assert b"set_param_schedule" in _lib.lib.mgadmm_last_error()
    m = re.match(r"mgadmm 0\.3\.(\d+) ", _lib.version())
    assert m and int(m.group(1)) >= 3, _lib.version()
    assert "0.3.3: mgadmm_solver_set_param_schedule" in raw
    assert _lib.Params._fields_[-1][0] == "admm_convergence" and _lib.History._fields_[-1][0] == "n_iters_per_sample"      # no struct grew


def test_launch_arguments_end_with_the_three_schedule_words():
    """sp_rows, sp_row0, sp_stride are the last members of LdsArgs, behind gset: no offset that existing code reads moves.
    (Brace-aware: the members carry `{}` initialisers.)"""
    txt = open(os.path.join(PKG, "csrc", "lds_args.h")).read()
    body = txt[txt.index("struct LdsArgs : LdsArgsCore"):]
    body = re.sub(r"//.*", "", body[:body.index("\n};")]).replace("{}", "")
    names = re.findall(r"(\w+)(?:\[[^\]]*\])?\s*[;,]", body)
    assert names[-6:] == ["off_node", "img_stride", "gset", "sp_rows", "sp_row0", "sp_stride"], names


# ------------------------------------------------------------------------------------------------ Python validation
ONES = np.ones((4, 3))


def _with(r, b, v):
    a = ONES.copy()
    a[r, b] = v
    return a


BAD = [
    (dict(param_schedule={"rho_x": [1, 1]}), "unknown key 'rho_x'"),
    (dict(param_schedule=[1, 2, 3]), "must be a dict"),
    (dict(param_schedule={"rho": np.ones((4, 2))}), r"shape \(K,\) or \(K, B = 3\)"),
    (dict(param_schedule={"rho": np.ones((4, 3, 1))}), r"shape \(K,\) or \(K, B = 3\)"),
    (dict(param_schedule={"rho": 1.0}), r"shape \(K,\) or \(K, B = 3\)"),
    (dict(param_schedule={"rho": np.ones((0, 3))}), "K >= 1"),
    (dict(param_schedule={"rho": ONES, "mu_u": np.ones((5, 3))}), "one number of rows"),
    (dict(param_schedule={"rho": ONES, "mu_u": np.ones(4)}), "one form"),
    (dict(param_schedule={"rho": _with(2, 1, 0.0)}), r"\['rho'\]\[2\]\[1\] = 0.0"),
    (dict(param_schedule={"rho_u": torch.from_numpy(_with(3, 2, -2.0))}), r"\['rho_u'\]\[3\]\[2\]"),
    (dict(param_schedule={"rho_d": [1.0, 1.0, 0.0]}), r"\['rho_d'\]\[2\] = 0.0"),
    (dict(param_schedule={"mu_d1": _with(0, 0, np.nan)}), r"\['mu_d1'\]\[0\]\[0\] is not finite"),
    (dict(param_schedule={"mu_d2": [1.0, np.inf]}), r"\['mu_d2'\]\[1\] is not finite"),
    (dict(param_schedule={"mu_u": _with(1, 2, -1e-9)}), r"\['mu_u'\]\[1\]\[2\]"),
    (dict(param_schedule={"mu_u": ONES}, sample_params={"mu_u": [1, 1, 1]}), r"\['mu_u'\] is given twice"),
    (dict(param_schedule={"rho": ONES}, schedule_start=-1), "schedule_start"),
    (dict(param_schedule={"rho": ONES}, schedule_start=1.5), "schedule_start"),
]


@pytest.mark.parametrize("kw, msg", BAD, ids=[m for _, m in BAD])
def test_schedules_are_validated_before_the_library_is_touched(kw, msg, monkeypatch):
    blk = _tiny()
    touched = []
    monkeypatch.setattr(type(blk), "_solver", lambda self, *a: touched.append(a))
    y = torch.ones(3, 12, 2, 1)
    with pytest.raises(ValueError, match=msg):
        blk.solve(y, **kw)
    if "schedule_start" not in kw:
        with pytest.raises(ValueError, match=msg):
            blk.combined_loop(y, print_info=False, **kw)
    assert touched == [] and blk._solvers == {}


def test_accepted_schedules():
    from mgadmm.ADMM import _check_param_schedule
    out, K, cols = _check_param_schedule({"mu_u": [0, 1, 2, 3], "rho": torch.tensor([1, 2, 3, 4])}, 3)       # mu = 0 is allowed, ints are
    assert list(out) == ["mu_u", "rho"] and (K, cols) == (4, 0)
    assert all(v.dtype == np.float64 and v.flags["C_CONTIGUOUS"] for v in out.values())
    out, K, cols = _check_param_schedule({"rho_d": np.asfortranarray(ONES * 2)}, 3, 7, {"rho": np.ones(3)})
    assert (K, cols) == (4, 3) and out["rho_d"].flags["C_CONTIGUOUS"] and out["rho_d"].shape == (4, 3)
    assert _check_param_schedule({}, 3) == ({}, 0, 0)
    # a (K, B) array with B = K is the per-sample form; (K,) the shared one
    assert _check_param_schedule({"rho": np.ones((3, 3))}, 3)[1:] == (3, 3)


# ------------------------------------------------------------------------------------------------ geometric_ramp
def test_geometric_ramp():
    from mgadmm.ADMM import geometric_ramp
    r = geometric_ramp(2.0, 1.5, 5)
    assert r.dtype == np.float64 and r.tolist() == [2.0, 3.0, 4.5, 6.75, 10.125]
    assert geometric_ramp(2.0, 1.5, 5, vmax=5).tolist() == [2.0, 3.0, 4.5, 5.0, 5.0]
    assert geometric_ramp(3.0, 1.0, 3).tolist() == [3.0, 3.0, 3.0] and geometric_ramp(4.0, 0.5, 3).tolist() == [4.0, 2.0, 1.0]
    assert geometric_ramp(1.0, 2.0, 1).tolist() == [1.0]
    for bad in ((0.0, 1.1, 3), (1.0, -1.0, 3), (1.0, 1.1, 0), (float("nan"), 1.1, 3), (1.0, 1.1, 2.5)):
        with pytest.raises(ValueError, match="geometric_ramp"):
            geometric_ramp(*bad)
    import mgadmm.ADMM as A
    assert "geometric_ramp" in A.__all__


# ------------------------------------------------------------------------------------------------ sweep
class _Stub:
    """solve() of an instance replaced: records what sweep() asks for and answers with tensors that name the sample."""

    def __init__(self, blk):
        self.blk, self.calls = blk, []

    def __call__(self, y, mask=None, sample_params=None, **kw):
        self.calls.append(dict(y=y.clone(), sp=sample_params, kw=kw))
        B = y.shape[0]
        x = y[:, :1, :1, :1].expand(B, 24, 2, 1).clone()
        self.blk.n_iters_per_sample = np.arange(B, dtype=np.int32)
        return x, (None, None), None, {}


def test_sweep_crosses_the_schedules_with_the_grid(monkeypatch):
    from mgadmm.ADMM import geometric_ramp
    blk = _tiny()
    stub = _Stub(blk)
    monkeypatch.setattr(blk, "solve", stub)
    W = 3
    y = torch.arange(W, dtype=torch.float32).reshape(W, 1, 1, 1).expand(W, 12, 2, 1).clone()
    ramps = [geometric_ramp(1.0, f, 5) for f in (1.0, 1.1)]
    mus = [np.full(5, 2.0), np.linspace(1, 3, 5), np.linspace(3, 1, 5)]
    x, n, sets = blk.sweep(y, {"mu_d1": [0.5, 4]}, schedules={"rho": ramps, "mu_u": mus})
    want = [(a, r, m) for a in (0.5, 4) for r in range(2) for m in range(3)]               # itertools.product order, grid keys first
    assert len(sets) == 12 and all(list(s) == ["mu_d1", "rho", "mu_u"] for s in sets)
    for s, (a, r, m) in zip(sets, want):
        assert s["mu_d1"] == a and np.array_equal(s["rho"], ramps[r]) and np.array_equal(s["mu_u"], mus[m])
    assert tuple(x.shape) == (12, W, 24, 2, 1) and n.shape == (12, W) and n.ravel().tolist() == list(range(12 * W))
    c = stub.calls[0]
    assert len(stub.calls) == 1 and set(c["kw"]) == {"return_state", "param_schedule"} and c["kw"]["return_state"] is False
    assert list(c["sp"]) == ["mu_d1"] and c["sp"]["mu_d1"] == [a for a, _, _ in want for _ in range(W)]
    ps = c["kw"]["param_schedule"]
    assert list(ps) == ["rho", "mu_u"] and ps["rho"].shape == (5, 12 * W)
    for p, (_, r, m) in enumerate(want):
        for w in range(W):                                   # sample p * W + w: set p on window w
            assert np.array_equal(ps["rho"][:, p * W + w], ramps[r]) and np.array_equal(ps["mu_u"][:, p * W + w], mus[m])
            assert float(c["y"][p * W + w, 0, 0, 0]) == w
    # in pieces: the columns follow the samples of the piece
    stub.calls.clear()
    blk.sweep(y, {"mu_d1": [0.5, 4]}, schedules={"rho": ramps, "mu_u": mus}, chunk=8)
    assert [cc["kw"]["param_schedule"]["rho"].shape for cc in stub.calls] == [(5, 8)] * 4 + [(5, 4)]
    assert np.array_equal(np.concatenate([cc["kw"]["param_schedule"]["mu_u"] for cc in stub.calls], 1), ps["mu_u"])
    # schedules alone
    stub.calls.clear()
    _, _, sets1 = blk.sweep(y, {}, schedules={"rho": ramps})
    assert len(sets1) == 2 and stub.calls[0]["sp"] == {} and stub.calls[0]["kw"]["param_schedule"]["rho"].shape == (5, 2 * W)


def test_sweep_without_schedules_passes_nothing_new(monkeypatch):
    blk = _tiny()
    stub = _Stub(blk)
    monkeypatch.setattr(blk, "solve", stub)
    y = torch.ones(2, 12, 2, 1)
    for kw in ({}, {"schedules": None}, {"schedules": {}}):
        stub.calls.clear()
        blk.sweep(y, {"mu_u": [1, 2]}, **kw)
        assert [c["kw"] for c in stub.calls] == [{"return_state": False}]


def test_sweep_refuses_bad_schedules():
    blk = _tiny()
    y = torch.ones(2, 12, 2, 1)
    with pytest.raises(ValueError, match="unknown schedule key"):
        blk.sweep(y, {}, schedules={"u_sigma": [np.ones(3)]})
    with pytest.raises(ValueError, match="given twice"):
        blk.sweep(y, {"rho": [1, 2]}, schedules={"rho": [np.ones(3)]})
    with pytest.raises(ValueError, match="one length K"):
        blk.sweep(y, {}, schedules={"rho": [np.ones(3), np.ones(4)]})
    with pytest.raises(ValueError, match="one length K"):
        blk.sweep(y, {}, schedules={"rho": [np.ones((3, 2))]})


# ------------------------------------------------------------------------------------------------ the twin discriminates
def test_the_table_of_the_tests():
    tab = pc.table()
    inf = pc.info()
    assert list(tab) == NAMES and all(v.shape == (12, 8) for v in tab.values())
    assert pc.K == 20 and pc.N_ROWS == 12 and pc.K > 16 > pc.N_ROWS               # the clamp and the launch boundary 16 + 4
    for nm in NAMES:
        assert (tab[nm][:, 0] == float(inf[nm])).all()                             # sample 0: equal rows
    assert np.allclose(tab["rho"][:, 3], float(inf["rho"]) * 1.2 ** np.arange(12), rtol=1e-15)
    assert tab["rho_u"][11, 4] == float(inf["rho_u"]) * 0.95 ** 11.0
    for b in pc.MU_SAMPLES:
        assert (tab["rho"][:, b] == float(inf["rho"])).all()
        assert tab["mu_u"][0, b] == 0.5 * inf["mu_u"] and tab["mu_u"][11, b] == 2 * inf["mu_u"]
        assert tab["mu_d1"][0, b] == 2 * inf["mu_d1"] and tab["mu_d1"][11, b] == 0.5 * inf["mu_d1"]
        assert tab["mu_d2"][0, b] == inf["mu_d2"] and tab["mu_d2"][11, b] == 3 * inf["mu_d2"]
    assert pc.scalars_of(tab, 3, 15)["rho"] == tab["rho"][11, 3] and pc.scalars_of(tab, 3, 2, first_row=8)["rho"] == tab["rho"][10, 3]
    pad = pc.padded(tab, 20)
    assert pad["rho"].shape == (20, 8) and (pad["rho"][12:] == tab["rho"][11]).all() and (pad["rho"][:12] == tab["rho"]).all()


@pytest.mark.parametrize("i", range(len(pc.CASES)), ids=pc.IDS)
def test_the_twin_discriminates(i):
    """The float64 twin under the table against (a) the constant-weight oracle: > 5e-3 = 500 x the float32 tolerance, and
    (b) the same schedule started one row later: > 5e-4 = 50 x the tolerance, on every sample whose rows differ; sample 0
    (equal rows) is the constant solve exactly.  A product that read a wrong row, or no row, cannot pass the GPU test
    against this twin."""
    twin = pc.twin_solutions(i)
    shifted = pc.twin_solutions(i, 1)
    const = pc.constant_solutions(i)
    worst_c, worst_s = np.inf, np.inf
    for b in range(8):
        x, o = twin[b]
        assert len(o.hist.p_res_list) == pc.K
        cg = [np.array(getattr(o.hist, nm)) for nm in ("CG_iter_x", "CG_iter_zu")]
        assert all((c > 0).all() and c.max() < 100 for c in cg), b                  # no solve of the twin hits the CG limit
        if b == 0:
            assert np.array_equal(x, const[b:b + 1]) and np.array_equal(x, shifted[b][0])
            continue
        worst_c, worst_s = min(worst_c, rel(x, const[b:b + 1])), min(worst_s, rel(x, shifted[b][0]))
    print("smallest difference: against constant weights", worst_c, "against the schedule shifted by one row", worst_s)
    assert worst_c > 5e-3 and worst_s > 5e-4, (worst_c, worst_s)


def test_the_twin_reads_the_row_of_the_iteration():
    """The property trick itself: 8 iterations, then 12 resumed from row 8, walk the rows of 20 iterations in one call."""
    o = pc.scheduled_oracle("knn", "None", {"rho": np.arange(1.0, 13.0)}, first_row=8)
    from oracle.admm_oracle import History
    o.hist = History()
    seen = []
    for _ in range(6):
        seen.append(o.rho)
        o.hist.p_res_list.append(0.0)
    assert seen == [9.0, 10.0, 11.0, 12.0, 12.0, 12.0]
    o.rho = 99.0                                             # the setter ignores assignments
    assert o.rho == 12.0 and o.mu_u == float(pc.info()["mu_u"])
