"""CPU checks of per-sample temporal band weights (mgadmm_solver_set_sample_bands, solve(band_params=...) /
solve(band_sets=...), sweep(skips=...)).  None of it needs a GPU.

  * tests/cpu/band_sets_check.cpp (AddressSanitizer + UBSan, a program of its own) over csrc/band_sets.h: every refusal and its
    message, the expansion with its zero padding columns, a padded narrow table against the native one;
  * the checks of mgadmm/band_args.py: shapes, ranges, both forms given, the table builder of 'skip';
  * the header's declaration, the ctypes mirror, the exported symbol, the version line; no struct grew;
  * the ABI calls of a solve with band arguments: set after the existing four, cleared first; none without them;
  * sweep() forming its cells with skips."""
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

import band_sets_cases as bc                  # noqa: E402


# ------------------------------------------------------------------------------------------------ the header
def test_band_sets_header_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "band_sets_check")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpu", "band_sets_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    got = json.loads(out.stdout)
    assert got == {"sets": 4, "B": 70, "T": 24, "skip": 6, "entries_read": 15 + 18 * 6, "feature": "sample_bands"}


def test_the_header_is_plain_cxx_and_solve_gate_is_untouched_by_it():
    txt = re.sub(r"//.*", "", open(os.path.join(PKG, "csrc", "band_sets.h")).read())
    assert "hip" not in txt.lower() and "getenv" not in txt
    gate = open(os.path.join(PKG, "csrc", "solve_gate.h")).read()
    assert "band_sets" not in gate and "sample_bands" not in gate          # the band decisions live in their own header


# ------------------------------------------------------------------------------------------------ ABI
def test_header_binding_symbol_and_version_agree():
    from mgadmm import _lib
    raw = open(os.path.join(ROOT, "include", "mgadmm.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"int mgadmm_solver_set_sample_bands\(mgadmm_solver\* s, int32_t n_sets, const float\* band_w\s*,\s*"
                     r"const int32_t\* set_of_sample\s*,\s*int32_t B\);", txt)
    res, args = _lib.SYMBOLS["mgadmm_solver_set_sample_bands"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int32]
    assert _lib.lib.mgadmm_solver_set_sample_bands.argtypes == args
    assert _lib.lib.mgadmm_solver_set_sample_bands(None, 0, None, None, 0) == _lib.ERR_INVALID
    assert b"set_sample_bands" in _lib.lib.mgadmm_last_error()
    m = re.match(r"mgadmm 0\.3\.(\d+) ", _lib.version())
    assert m and int(m.group(1)) >= 5, _lib.version()
    assert "0.3.5: mgadmm_solver_set_sample_bands" in raw
    # no struct grew
    assert _lib.Params._fields_[-1][0] == "admm_convergence" and _lib.History._fields_[-1][0] == "n_iters_per_sample"
    assert _lib.GraphDesc._fields_[-1][0] == "device" and [f[0] for f in _lib.State._fields_][-1] == "gamma_d"
    assert C.sizeof(_lib.AdaptiveRho) == 8 + 16 + 48 and C.sizeof(_lib.SampleParams) == 6 * C.sizeof(C.c_void_p)


def test_launch_arguments_grow_behind_everything_that_exists():
    txt = open(os.path.join(PKG, "csrc", "lds_args.h")).read()
    body = txt[txt.index("struct LdsArgs : LdsArgsCore"):]
    body = re.sub(r"//.*", "", body[:body.index("\n};")])
    assert body.rstrip().endswith("const int* bset{nullptr};")
    assert body.index("sp_stride") < body.index("bset") and "band" not in body[:body.index("sp_stride")]


# ------------------------------------------------------------------------------------------------ Python validation
def _line(skip=bc.WIDTH, **kw):
    return bc.instance("None", skip, **kw)


def _knn():
    import graph_sets_cases as gc
    return gc.instance("knn", "None", *gc.pairs()[1])


def _untouched(blk, monkeypatch):
    touched = []
    monkeypatch.setattr(type(blk), "_solver", lambda self, *a: touched.append(a))
    return touched


T, WIDTH = 24, bc.WIDTH
GOOD = np.stack(bc.tables())
BAD = [
    (dict(band_of_sample=[0, 0, 0]), "band_of_sample needs band_sets"),
    (dict(band_params={"skip": [1, 2, 3]}, band_sets=[GOOD[0]]), "exclude each other"),
    (dict(band_params=[1, 2, 3]), "must be a dict"),
    (dict(band_params={"hops": [1, 2, 3]}), "unknown key 'hops'"),
    (dict(band_params={}), "needs 'skip'"),
    (dict(band_params={"skip": [1, 2]}), "B = 3 integers"),
    (dict(band_params={"skip": [[1, 2, 3]]}), "B = 3 integers"),
    (dict(band_params={"skip": [1.0, 2.0, 3.0]}), "B = 3 integers"),
    (dict(band_params={"skip": [1, 0, 3]}), r"band_params\['skip'\]\[1\] = 0 outside \[1, skip_connection = 6\]"),
    (dict(band_params={"skip": torch.tensor([1, 2, 7])}), r"band_params\['skip'\]\[2\] = 7 outside"),
    (dict(band_sets=[], band_of_sample=[0, 0, 0]), "band_sets is empty"),
    (dict(band_sets=[GOOD[0]]), "needs band_of_sample"),
    (dict(band_sets=[GOOD[0][:, :3]], band_of_sample=[0, 0, 0]), r"band_sets\[0\] has shape \(24, 3\)"),
    (dict(band_sets=[GOOD[0], GOOD[1][:-1]], band_of_sample=[0, 0, 0]), r"band_sets\[1\] has shape \(23, 6\)"),
    (dict(band_sets=[GOOD[0]], band_of_sample=[0, 0]), "B = 3 integers"),
    (dict(band_sets=[GOOD[0]], band_of_sample=[0.0, 0.0, 0.0]), "B = 3 integers"),
    (dict(band_sets=[GOOD[0]], band_of_sample=[0, 1, 0]), r"band_of_sample\[1\] = 1 out of range for 1 band sets"),
    (dict(band_sets=[GOOD[0], GOOD[1]], band_of_sample=[0, -1, 0]), "out of range"),
]


@pytest.mark.parametrize("kw, msg", BAD, ids=[re.sub(r"\W+", "_", m)[:40] for _, m in BAD])
def test_band_arguments_are_validated_before_the_library_is_touched(kw, msg, monkeypatch):
    blk = _line()
    touched = _untouched(blk, monkeypatch)
    y = torch.ones(3, 12, blk.n_nodes, 1)
    with pytest.raises(ValueError, match=msg):
        blk.solve(y, **kw)
    with pytest.raises(ValueError, match=msg):
        blk.combined_loop(y, print_info=False, **kw)
    assert touched == [] and blk._solvers == {}


def test_non_finite_entries_count_only_where_they_are_read(monkeypatch):
    from mgadmm import band_args
    blk = _line()
    tab = GOOD[4].copy()
    tab[0, :] = np.nan
    tab[2, 2:] = np.inf                      # row t reads the hops s < min(t, skip)
    tables, bos = band_args.check_band_args(blk, None, [tab], [0, 0, 0], 3)
    assert tables.shape == (1, T, WIDTH) and bos.tolist() == [0, 0, 0]
    tab[2, 1] = np.nan
    with pytest.raises(ValueError, match=r"band_sets\[0\]\[2\]\[1\] is not finite"):
        band_args.check_band_args(blk, None, [tab], [0, 0, 0], 3)


def test_refused_for_an_instance_without_a_line_graph(monkeypatch):
    blk = _knn()
    touched = _untouched(blk, monkeypatch)
    y = torch.ones(3, 12, blk.n_nodes, 1)
    for kw in (dict(band_params={"skip": [1, 1, 1]}), dict(band_sets=[GOOD[0]], band_of_sample=[0, 0, 0])):
        with pytest.raises(ValueError, match="no line graph"):
            blk.solve(y, **kw)
    with pytest.raises(ValueError, match="needs a line-graph instance"):
        blk.sweep(y, {"mu_u": [1, 2]}, skips=[1])
    assert touched == []
    # the earlier checks answer first: sample_params, then the graph arguments, then the band arguments
    with pytest.raises(ValueError, match="sample_params"):
        blk.solve(y, sample_params={"rho": [1, 0, 1]}, band_params={"skip": [1, 1, 1]})
    with pytest.raises(ValueError, match="graph_of_sample needs graph_sets"):
        blk.solve(y, graph_of_sample=[0, 0, 0], band_of_sample=[0, 0, 0])


def test_the_skip_tables_and_the_set_of_every_sample():
    """band_params -> the distinct intervals in order of first appearance, each the table of utils.skip_connection_tables
    zero-padded to the instance's width; on the entries an operator reads it is the native table."""
    from mgadmm import band_args, utils
    blk = _line()
    tables, bos = band_args.check_band_args(blk, {"skip": [3, 1, 3, 6, 1]}, None, None, 5)
    assert tables.dtype == np.float32 and tables.flags.c_contiguous and tables.shape == (3, T, WIDTH)
    assert bos.dtype == np.int32 and bos.tolist() == [0, 1, 0, 2, 1]
    for tab, s in zip(tables, (3, 1, 6)):
        native = utils.skip_connection_tables(1, T, s)[0][:, :, 0].numpy()
        assert np.array_equal(tab[:, :s], native) and not tab[:, s:].any()
        assert np.array_equal(tab, bc.uniform_table(s)) and np.array_equal(native, bc.uniform_table(s, s))
    assert np.array_equal(tables[2], blk.d_ew[:, :, 0].numpy())           # the full width is the instance's own table
    narrow = _line(3)
    with pytest.raises(ValueError, match=r"= 4 outside \[1, skip_connection = 3\]"):
        band_args.check_band_args(narrow, {"skip": [1, 4]}, None, None, 2)
    with pytest.raises(ValueError, match="skip = 0 outside"):
        band_args.skip_table(T, 0, 3)
    assert band_args.check_band_args(blk, None, None, None, 5) is None
    # the low-level form: tensors and arrays, any integer dtype of the index
    tables, bos = band_args.check_band_args(blk, None, [torch.from_numpy(GOOD[4]), GOOD[1].astype(np.float64)], np.array([1, 0, 1], dtype=np.uint8), 3)
    assert tables.dtype == np.float32 and np.array_equal(tables[0], GOOD[4]) and bos.dtype == np.int32 and bos.tolist() == [1, 0, 1]
    for skips, msg in (([], "empty"), ([1, 7], r"skips\[1\] = 7 outside"), ([0], r"skips\[0\] = 0 outside"), ([1.5], "integers"), (3, "integers")):
        with pytest.raises(ValueError, match=msg):
            band_args.check_skips(blk, skips)
    assert band_args.check_skips(blk, np.array([6, 1])) == [6, 1]


# ------------------------------------------------------------------------------------------------ the ABI calls of a solve
class _Recorder:
    """Stands in for the library: records the setter calls and the solve, returns OK (or `refuse` for one name)."""

    def __init__(self, refuse=None):
        self.calls, self.refuse = [], refuse

    def __getattr__(self, name):
        def call(*a):
            if name.startswith("mgadmm_solver_set_sample") or name in ("mgadmm_solver_set_param_schedule", "mgadmm_solver_set_adaptive_rho", "mgadmm_solve"):
                self.calls.append((name, a[1] if name != "mgadmm_solve" else None))
            if name == "mgadmm_last_error":
                return b"refused"
            return -4 if name == self.refuse else 0
        return call


def _scope_calls(monkeypatch, args, refuse=None):
    from mgadmm import _lib, solve_args
    rec = _Recorder(refuse)
    monkeypatch.setattr(_lib, "lib", rec)
    with solve_args.solve_scope(None, None, 1, 3, args):
        rec.mgadmm_solve()
    return [n for n, _ in rec.calls], rec.calls


def test_the_band_table_is_set_after_the_existing_setters_and_cleared_first(monkeypatch):
    from mgadmm import _lib, solve_args
    blk = _line()
    kw = dict(sample_params={"rho": [1.0, 2.0, 3.0]}, param_schedule={"mu_u": np.ones((4, 3))}, band_params={"skip": [1, 2, 2]})
    args = solve_args.parse_solve_args(blk, 3, **kw)
    assert args.bs is not None and args.bs[0].shape == (2, T, WIDTH) and args.bs[1].tolist() == [0, 1, 1]
    names, calls = _scope_calls(monkeypatch, args)
    sp, sch, band = "mgadmm_solver_set_sample_params", "mgadmm_solver_set_param_schedule", "mgadmm_solver_set_sample_bands"
    assert names == [sp, sch, band, "mgadmm_solve", band, sch, sp]
    band_calls = [a for n, a in calls if n == band]
    assert band_calls == [2, 0]                                   # n_sets: set with two tables, cleared with 0
    # adaptive_rho and the band table: the band table last, cleared first
    args = solve_args.parse_solve_args(blk, 3, adaptive_rho={"every": 2}, band_params={"skip": [1, 2, 2]})
    names, _ = _scope_calls(monkeypatch, args)
    assert names == ["mgadmm_solver_set_adaptive_rho", band, "mgadmm_solve", band, "mgadmm_solver_set_adaptive_rho"]
    # a set call that refuses raises and is not cleared; what was set before it is
    with pytest.raises(_lib.MgadmmError):
        _scope_calls(monkeypatch, args, refuse=band)
    # without band arguments: exactly the calls there were
    args = solve_args.parse_solve_args(blk, 3, sample_params={"rho": [1.0, 2.0, 3.0]})
    assert args.bs is None and _scope_calls(monkeypatch, args)[0] == [sp, "mgadmm_solve", sp]
    assert _scope_calls(monkeypatch, solve_args.parse_solve_args(blk, 3))[0] == ["mgadmm_solve"]


def test_new_checks_live_in_band_args():
    """ADMM.py and solve_args.py got no raise statement for the band arguments: every message about them comes from band_args.py."""
    for name in ("ADMM.py", "solve_args.py"):
        src = open(os.path.join(PKG, "mgadmm", name)).read()
        for m in re.finditer(r"raise \w+\((.*)", src):
            assert "band" not in m.group(1) and "skips" not in m.group(1), (name, m.group(0))
    assert "raise ValueError" in open(os.path.join(PKG, "mgadmm", "band_args.py")).read()


# ------------------------------------------------------------------------------------------------ sweep
def test_sweep_crosses_the_skips_with_the_grid_after_its_keys(monkeypatch):
    blk = _line()
    calls = []

    def solve(y, mask=None, sample_params=None, band_params=None, **kw):
        calls.append(dict(sp=sample_params, bp=band_params, kw=kw))
        B = y.shape[0]
        code = torch.tensor([100.0 * sample_params["mu_d1"][b] + band_params["skip"][b] for b in range(B)])
        blk.n_iters_per_sample = np.arange(B, dtype=np.int32)
        return (y[:, :1, :1, :1] * 1000 + code.reshape(B, 1, 1, 1)).expand(B, 24, 2, 1).clone(), (None, None), None, {}

    monkeypatch.setattr(blk, "solve", solve)
    W = 3
    y = torch.arange(W, dtype=torch.float32).reshape(W, 1, 1, 1).expand(W, 12, 2, 1).clone()
    x, n, sets = blk.sweep(y, {"mu_d1": [1, 2]}, skips=[1, 3, 6])
    assert sets == [dict(mu_d1=m, skip=s) for m in (1, 2) for s in (1, 3, 6)]
    assert tuple(x.shape) == (6, W, 24, 2, 1) and n.shape == (6, W) and n.ravel().tolist() == list(range(6 * W))
    assert len(calls) == 1 and calls[0]["kw"] == {"return_state": False} and list(calls[0]["bp"]) == ["skip"]
    assert calls[0]["bp"]["skip"] == [s for m in (1, 2) for s in (1, 3, 6) for _ in range(W)]
    for p, s in enumerate(sets):
        for w in range(W):
            assert float(x[p, w, 0, 0, 0]) == 1000 * w + 100 * s["mu_d1"] + s["skip"], (p, w)
    # with schedules: grid keys, schedule keys, then 'skip'
    calls.clear()

    def solve2(y, mask=None, sample_params=None, **kw):
        calls.append(kw)
        blk.n_iters_per_sample = np.zeros(y.shape[0], np.int32)
        return y.expand(y.shape[0], 12, 2, 1).clone(), None, None, {}

    monkeypatch.setattr(blk, "solve", solve2)
    _, _, sets = blk.sweep(y, {"mu_u": [1.0]}, schedules={"rho": [np.ones(2), 2 * np.ones(2)]}, skips=[2, 1], chunk=6)
    assert [list(s) for s in sets] == [["mu_u", "rho", "skip"]] * 4 and [s["skip"] for s in sets] == [2, 1, 2, 1]
    assert [c["band_params"]["skip"] for c in calls] == [[2, 2, 2, 1, 1, 1], [2, 2, 2, 1, 1, 1]]
    # without skips solve() is called as before: no band argument at all
    calls.clear()
    blk.sweep(y, {"mu_u": [1, 2]})
    assert calls == [{"return_state": False}]
