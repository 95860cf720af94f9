"""CPU checks of the adaptive penalties (mgadmm_solver_set_adaptive_rho, solve(adaptive_rho=..., adaptive_start=...)).  None of
it needs a GPU.

  * tests/cpu/lds_adapt_check.cpp (AddressSanitizer + UBSan, a program of its own) on csrc/lds_adapt.h: the branches of the
    rule, the clamps, NaN and 0 / 0, the ablations; adapt_J, the steps of a solve and the rows they write against loops
    written out there; the refusals by name; a rule that never steps leaving fill_records of the start weights;
  * the rule restated in numpy (tests/adaptive_rho_cases.py) against the program on 10^4 random inputs, exactly;
  * the header's declarations, the version line, the ctypes mirror, the exported symbols;
  * lds_schedule.h is what it was before the feature, and the kernels of lds_kernels.h compile to the recorded instructions;
  * validation in Python before the library is touched;
  * the float64 twin: every decision at least 1 % from its threshold, steps in both directions, and a solution that differs
    from the constant-penalty one by >= 1e-2 per sample, so a kernel that ignores the table cannot pass a 1e-5 comparison."""
import ctypes as C
import hashlib
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

import adaptive_rho_cases as ac               # noqa: E402
from helpers import _tiny, rel                # noqa: E402


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("lds_adapt") / "lds_adapt_check")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpu", "lds_adapt_check.cpp"), "-o", exe])
    return exe


# ------------------------------------------------------------------------------------------------ the header's own check
def test_rule_and_planning_under_the_sanitizers(check_exe):
    out = subprocess.run([check_exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    res = json.loads(out.stdout)
    assert res["cases"] > 10000 and res["steps"] > 10000
    assert res["refusals"] == [
        "adaptive_rho: every = 0 outside [1, 16]", "adaptive_rho: every = 17 outside [1, 16]",
        "adaptive_rho: mu = 1, should be > 1 (and < 1e150)", "adaptive_rho: mu = nan, should be > 1 (and < 1e150)",
        "adaptive_rho: tau = 1, should be > 1 (and < 1e150)",
        "adaptive_rho: rho_min[rho] = 0, rho_max[rho] = 1000, should be 0 < rho_min <= rho_max (finite)",
        "adaptive_rho: rho_min[rho] = 2, rho_max[rho] = 1, should be 0 < rho_min <= rho_max (finite)",
        "adaptive_rho: start = -4 is negative", "adaptive_rho: start = 6 is no multiple of every = 4",
        "adaptive_rho: until = -1 is negative (0: no limit)"]


def test_numpy_rule_equals_the_header_on_random_inputs(check_exe, tmp_path):
    """10^4 records: penalties and residual sums log-uniform over 12 decades, a fifth of the records ON a threshold (pri2 =
    m2 * s2 formed with the rule's own products), some sums 0 or NaN, narrow clamps on a third."""
    rng = np.random.default_rng(11)
    n = 10000
    rec = np.zeros((n, 19))
    rec[:, 0:3] = 10.0 ** rng.uniform(-3, 3, (n, 3))
    rec[:, 3:9] = 10.0 ** rng.uniform(-6, 6, (n, 6))
    rec[:, 9:11] = rng.integers(0, 2, (n, 2))
    rec[:, 11] = rng.choice([1.5, 2.0, 10.0, 1e30], n)
    rec[:, 12] = rng.choice([2.0, 1.5, 1.1, 3.0], n)
    rec[:, 13:16], rec[:, 16:19] = 1e-6, 1e6
    narrow = rng.random(n) < 1 / 3
    rec[narrow, 13:16] = rec[narrow, 0:3] * rng.uniform(0.6, 1.0, (int(narrow.sum()), 3))
    rec[narrow, 16:19] = rec[narrow, 0:3] * rng.uniform(1.0, 1.7, (int(narrow.sum()), 3))
    on = rng.random(n) < 0.2
    for f, (ip, idd) in enumerate(((5, 6), (3, 4), (7, 8))):      # columns of the pair of rho, rho_u, rho_d
        r, m2 = rec[:, f], rec[:, 11] * rec[:, 11]
        rec[on, ip] = (m2 * (r * r * rec[:, idd]))[on]
    rec[rng.random(n) < 0.02, 3] = 0.0
    rec[rng.random(n) < 0.02, 4] = 0.0
    rec[rng.random(n) < 0.02, 5] = np.nan
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    rec.tofile(fin)
    subprocess.check_call([check_exe, "rule", fin, fout])
    got = np.fromfile(fout).reshape(n, 3)
    want = np.empty((n, 3))
    want[:, 1] = ac.balance(rec[:, 1], rec[:, 3], rec[:, 4], rec[:, 11], rec[:, 12], rec[:, 14], rec[:, 17])
    want[:, 0] = np.where(rec[:, 9] != 0, ac.balance(rec[:, 0], rec[:, 5], rec[:, 6], rec[:, 11], rec[:, 12], rec[:, 13], rec[:, 16]), rec[:, 0])
    want[:, 2] = np.where(rec[:, 10] != 0, ac.balance(rec[:, 2], rec[:, 7], rec[:, 8], rec[:, 11], rec[:, 12], rec[:, 15], rec[:, 18]), rec[:, 2])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    moved = got != rec[:, 0:3]
    assert 0.2 < moved.mean() < 0.8 and (got > rec[:, 0:3]).any() and (got < rec[:, 0:3]).any()
    # and ac.step, the form the GPU tests use, on a batch
    sums = np.zeros((11, 64))
    sums[1:7] = rec[:64, 3:9].T
    w = ac.step({"rho": rec[:64, 0], "rho_u": rec[:64, 1], "rho_d": rec[:64, 2]}, sums, "None", 2.0, 2.0)
    for f, nm in enumerate(("rho", "rho_u", "rho_d")):
        ip, idd = {"rho": (3, 4), "rho_u": (1, 2), "rho_d": (5, 6)}[nm]
        assert np.array_equal(w[nm], ac.balance(rec[:64, f], sums[ip], sums[idd], 2.0, 2.0))
    big = np.zeros((11, 1))
    big[[1, 3, 5]] = 1e9                              # every primal residual dominates
    one = {"rho": 1.0, "rho_u": 1.0, "rho_d": 1.0}
    assert {k: float(np.ravel(v)[0]) for k, v in ac.step(one, big, "None", 2.0, 2.0).items()} == {"rho": 2.0, "rho_u": 2.0, "rho_d": 2.0}
    assert {k: float(np.ravel(v)[0]) for k, v in ac.step(one, big, "DGLR", 2.0, 2.0).items()} == {"rho": 2.0, "rho_u": 2.0, "rho_d": 1.0}
    assert {k: float(np.ravel(v)[0]) for k, v in ac.step(one, big, "DGTV", 2.0, 2.0).items()} == {"rho": 1.0, "rho_u": 2.0, "rho_d": 2.0}


def test_the_headers_are_plain_cxx():
    for name in ("lds_adapt.h", "lds_param_table.h"):
        txt = re.sub(r"//.*", "", open(os.path.join(PKG, "csrc", name)).read())
        assert "hip" not in txt.lower() and "getenv" not in txt, name
    txt = open(os.path.join(PKG, "csrc", "lds_param_table.h")).read()
    assert "MG_HD inline LhsDef lhs_def_of(" in txt and "MG_HD inline LdsSampleParams record_of(" in txt
    rule = re.sub(r"//.*", "", open(os.path.join(PKG, "csrc", "lds_adapt.h")).read())
    body = rule[rule.index("inline double balance("):rule.index("inline void step(")]
    assert "/" not in body and "+" not in body and "fma" not in body         # multiplications, comparisons, selects


@pytest.fixture(scope="module")
def kernel_isa():
    """tools/kernel_isa.py and the manifest of the tree under test: the three LDS units compiled once, side by side."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa as ki
    golden = json.load(open(ki.GOLDEN))
    if ki.hipcc_version() != golden["hipcc"]:
        pytest.skip(f"the recorded kernels are those of '{golden['hipcc']}'; this compiler is '{ki.hipcc_version()}'")
    return ki, golden, ki.manifest(ROOT)


def test_the_kernels_and_the_schedule_are_untouched(kernel_isa):
    """lds_schedule.h byte for byte; every k_admm_lds / k_admm_lds_ps / k_admm_lds_pp instance compiles to the instructions,
    registers, spills and scratch recorded in tests/golden/lds_kernel_isa.json (a change that means to move a kernel
    regenerates the file with `python tools/kernel_isa.py`, and the diff names the kernels that moved)."""
    sha = "9b432bec77744dd2aa1fcde80ec11a8859a8c98b899b76242606e772e6866f5e"
    assert hashlib.sha256(open(os.path.join(PKG, "csrc", "lds_schedule.h"), "rb").read()).hexdigest() == sha, "lds_schedule.h"
    ki, golden, here = kernel_isa
    assert len(golden["kernels"]) == len(here["kernels"]) == 135
    assert {r["unit"] for r in golden["kernels"]} == set(ki.LDS_UNITS)
    moved = ki.difference(golden, here)
    assert here["kernels"] == golden["kernels"] and not moved, "\n" + "\n".join(moved)


# ------------------------------------------------------------------------------------------------ ABI
def test_header_binding_and_symbols_agree():
    from mgadmm import _lib
    raw = open(os.path.join(ROOT, "include", "mgadmm.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"typedef struct \{([^{}]*)\} mgadmm_adaptive_rho;", txt)
    assert m and re.findall(r"(\w+)(?:\[3\])?\s*[,;]", m.group(1)) == ["every", "until", "mu", "tau", "rho_min", "rho_max"]
    assert re.search(r"int mgadmm_solver_set_adaptive_rho\(mgadmm_solver\* s, const mgadmm_adaptive_rho\* ar, int32_t start\);", txt)
    assert re.search(r"int mgadmm_solver_get_adaptive_history\(mgadmm_solver\* s, int32_t B, double\* rho_hist, int32_t max_periods, "
                     r"int32_t\* n_periods\);", txt)
    assert "0.3.4: mgadmm_solver_set_adaptive_rho" in raw
    m = re.match(r"mgadmm 0\.3\.(\d+) ", _lib.version())
    assert m and int(m.group(1)) >= 4, _lib.version()
    res, args = _lib.SYMBOLS["mgadmm_solver_set_adaptive_rho"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(_lib.AdaptiveRho), C.c_int32]
    assert [f[0] for f in _lib.AdaptiveRho._fields_] == ["every", "until", "mu", "tau", "rho_min", "rho_max"]
    assert C.sizeof(_lib.AdaptiveRho) == 8 + 16 + 48
    assert _lib.lib.mgadmm_solver_set_adaptive_rho(None, None, 0) == _lib.ERR_INVALID
    assert b"set_adaptive_rho" in _lib.lib.mgadmm_last_error()
    assert _lib.lib.mgadmm_solver_get_adaptive_history(None, 1, None, 0, None) == _lib.ERR_INVALID
    assert _lib.Params._fields_[-1][0] == "admm_convergence" and _lib.History._fields_[-1][0] == "n_iters_per_sample"      # no struct grew


# ------------------------------------------------------------------------------------------------ Python validation
BAD = [
    (dict(adaptive_rho=[4, 10, 2]), "must be a dict"),
    (dict(adaptive_rho={"every": 4, "nu": 2}), "unknown key 'nu'"),
    (dict(adaptive_rho={"mu": 10}), "needs 'every'"),
    (dict(adaptive_rho={"every": 0}), r"every = 0 outside \[1, 16\]"),
    (dict(adaptive_rho={"every": 17}), r"every = 17 outside \[1, 16\]"),
    (dict(adaptive_rho={"every": 4, "mu": 1.0}), "should both be > 1"),
    (dict(adaptive_rho={"every": 4, "tau": 0.5}), "should both be > 1"),
    (dict(adaptive_rho={"every": 4, "until": -1}), "until = -1 is negative"),
    (dict(adaptive_rho={"every": 4, "rho_min": 0.0}), r"rho_min\[rho\] = 0.0"),
    (dict(adaptive_rho={"every": 4, "rho_min": 2.0, "rho_max": [3, 1, 3]}), r"rho_min\[rho_u\] = 2.0, rho_max\[rho_u\] = 1.0"),
    (dict(adaptive_rho={"every": 4, "rho_max": [1, 2]}), "three numbers"),
    (dict(adaptive_rho={"every": 4, "rho_max": {"mu_u": 1}}), "unknown keys"),
    (dict(adaptive_rho={"every": 4}, adaptive_start=6), "adaptive_start = 6 must be a non-negative multiple of every = 4"),
    (dict(adaptive_rho={"every": 4}, adaptive_start=-4), "adaptive_start = -4"),
    (dict(adaptive_rho={"every": 4}, param_schedule={"rho": [1.0, 2.0]}), "exclude each other"),
]


@pytest.mark.parametrize("kw, msg", BAD, ids=[m[:24] for _, m in BAD])
def test_python_refuses_before_the_library_is_touched(kw, msg):
    blk = _tiny()
    with pytest.raises(ValueError, match=msg):
        blk.solve(torch.ones(3, 12, 2, 1), **kw)
    assert blk._solvers == {} and blk.rho_history is None


def test_python_forms_the_struct():
    from mgadmm.ADMM import _check_adaptive_rho
    ar, start = _check_adaptive_rho({"every": 4}, 8)
    assert (ar.every, ar.until, ar.mu, ar.tau, start) == (4, 0, 10.0, 2.0, 8)
    assert list(ar.rho_min) == [1e-6] * 3 and list(ar.rho_max) == [1e6] * 3
    ar, _ = _check_adaptive_rho({"every": 2, "mu": 3, "tau": 1.5, "until": 12, "rho_min": {"rho_u": 0.5}, "rho_max": [4, 5, 6]})
    assert (ar.every, ar.until, ar.mu, ar.tau) == (2, 12, 3.0, 1.5)
    assert list(ar.rho_min) == [1e-6, 0.5, 1e-6] and list(ar.rho_max) == [4.0, 5.0, 6.0]


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("i", range(len(ac.CASES)), ids=ac.IDS)
def test_twin_decisions_are_far_from_their_thresholds_and_the_solution_moves(i):
    every, mu, tau = ac.triple(i)
    twins, xc = ac.twin_solutions(i, every, mu, tau), ac.constant_solutions(i)
    margin = min(min(o.ad_margins) for _, o in twins)
    dirs = [d for _, o in twins for d in o.ad_dirs]
    print(ac.IDS[i], (every, mu, tau), "smallest margin", np.expm1(margin), "up", sum(d > 0 for d in dirs), "down", sum(d < 0 for d in dirs))
    assert margin >= np.log(1 + ac.MARGIN) and any(d > 0 for d in dirs) and any(d < 0 for d in dirs)
    assert (every, mu, tau) == [(4, 1.25, 2.0), (4, 1.25, 2.0), (4, 1.25, 2.0), (4, 1.5, 4.0)][i]      # the module docstring's record
    for b, (x, o) in enumerate(twins):
        d = rel(x, xc[b:b + 1])
        print("  sample", b, "adaptive against constant penalties", d)
        assert d >= 1e-2, (b, d)
        hist = ac.twin_history(o)
        lo, hi = ac.twin_clamps(i)
        assert (hist >= np.array(lo)).all() and (hist <= np.array(hi)).all()
        assert hist.shape == (1 + ac.K // every, 3) and (hist[0] == [float(ac.info()[nm]) for nm in ac.NAMES[:3]]).all()
        for nm in ("CG_iter_x", "CG_iter_zu", "CG_iter_zd"):
            assert np.max(getattr(o.hist, nm) or [0]) < 100


def test_a_triple_that_cannot_meet_the_conditions_raises(monkeypatch):
    monkeypatch.setattr(ac, "MARGIN", 0.9)            # no decision of a real run is a factor 1.9 from both thresholds
    ac.triple.cache_clear()
    with pytest.raises(RuntimeError, match="no .every, mu, tau."):
        ac.triple(0)
    ac.triple.cache_clear()
