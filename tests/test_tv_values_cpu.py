"""Time-varying edge weights without a GPU: the host header of the per-slice tables on the CPU, the refusals of the new entry
point that need no graph, the shape errors of ``ADMM_algorithm(time_varying=True)`` and today's refusal with the default.

tests/cpu/tv_values_check.cpp (built with AddressSanitizer + UBSan, run as a program of its own) checks the per-slice transposes
against dense transposes, the permutation round trip, and that for every (operator, t, row, GW) the slice index and the highest
entry offset the row kernel forms stay inside the table's allocation, T = 2 included."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import tv_cases as tc
from conftest import PKG, ROOT

CSRC = os.path.join(PKG, "csrc")


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("tv") / "tv_values_check")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpu", "tv_values_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads(out.stdout)


def test_the_table_check_is_clean_under_asan_and_ubsan(got):
    assert got["failed"] == 0 and got["checks"] > 1000 and got["offsets"] > 5000


def test_the_header_is_plain_cpp_and_the_kernel_and_launch_site_use_its_rule():
    text = open(os.path.join(CSRC, "tv_values.h")).read()
    assert "hip/" not in text and "__global__" not in text and "getenv" not in text
    kern = open(os.path.join(CSRC, "stream_tv_kernels.h")).read()
    assert "tv::slice_of(t, op.shift, op.n_slices)" in kern and not re.search(r"^struct Epi", kern, re.M)
    assert not re.search(r"k_(rows|tile|cldr)<", kern)
    # the twin exists for the epilogues that run with a spatial operator only
    eng = open(os.path.join(CSRC, "engine.h")).read()
    launch = eng[eng.index("op.val_t != nullptr"):eng.index("k_rows_tv<S, VEC, Epi, GW>")]
    assert "is_elementwise<Epi>::value" in launch


def test_set_time_weights_refuses_a_null_graph_without_a_gpu():
    from mgadmm import _lib
    assert "0.3.6" in _lib.version()
    v = np.ones((2, 3), dtype=np.float32)
    rc = _lib.lib.mgadmm_graph_set_time_weights(None, v.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 2, None, 0)
    assert rc == _lib.ERR_INVALID and b"graph_set_time_weights: null graph" in _lib.lib.mgadmm_last_error()


def test_python_shape_errors_name_the_table_and_both_shapes():
    from mgadmm.time_tables import table_slices
    g = tc.g11()
    T = 6
    cl, u, d = tc.tables("knn", 24)
    for nm, kw, shape, want in (("u_ew", dict(u_ew=u[:5], d_ew=d[:T - 1]), (5, 30, 4), (6, 30, 4)),
                                ("d_ew", dict(u_ew=u[:T], d_ew=d[:T]), (6, 30, 5), (5, 30, 5))):
        blk = tc.make_tv_product("knn", T, 3, tc.info_ops(), **kw)
        with pytest.raises(ValueError) as e:
            table_slices(getattr(blk, nm), nm, T if nm == "u_ew" else T - 1)
        assert nm in str(e.value) and str(shape) in str(e.value) and str(want) in str(e.value)
    assert int(g["T"]) == 24


def test_slices_collapse_when_equal_and_the_hook_keeps_them(monkeypatch):
    from mgadmm.time_tables import table_slices
    T = 4
    cl, u, d = tc.tables("knn", T)
    blk = tc.make_tv_product("knn", T, 2, tc.info_ops())
    assert len(table_slices(blk.u_ew, "u_ew", T)) == T and len(table_slices(blk.d_ew, "d_ew", T - 1)) == T - 1
    rep = torch.from_numpy(u[:1]).repeat(T, 1, 1)
    assert table_slices(rep, "u_ew", T) is None and table_slices(rep[0], "u_ew", T) is None
    monkeypatch.setenv("MGADMM_TV_KEEP", "1")
    kept = table_slices(rep, "u_ew", T)
    assert len(kept) == T and all(torch.equal(k, rep[0]) for k in kept)
    assert len(table_slices(rep[0], "u_ew", T)) == T
    # the flag is part of the table key: switching it rebuilds the device graph
    k1 = blk._table_key()
    blk.time_varying = False
    assert blk._table_key() != k1


def test_default_keeps_todays_refusal():
    from mgadmm.ADMM import ADMM_algorithm
    T = 4
    blk = tc.make_tv_product("knn", T, 2, tc.info_ops(), time_varying=False)
    assert blk.time_varying is False
    with pytest.raises(NotImplementedError, match="u_ew varies over the time axis"):      # before anything touches the device
        blk._make_graph(1, blk.u_ew, blk.d_ew)
    for nm in ("u_ew", "d_ew"):
        with pytest.raises(NotImplementedError) as e:
            ADMM_algorithm._time_invariant(getattr(blk, nm), nm)
        assert str(e.value) == (f"{nm} varies over the time axis; only time-expanded repeats of one (N, k) table "
                                "(expand_time_dimension, utils.py:294-295) are supported")
