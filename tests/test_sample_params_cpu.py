"""CPU checks of per-sample ADMM weights (mgadmm_solver_set_sample_params, ADMM_algorithm.solve(sample_params=...), sweep):
the declaration in the header and its ctypes mirror, the exported symbol, one k_admm_lds_pp instance per k_admm_lds instance,
the validation in Python and the order in which sweep() forms its batch.  None of it needs a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
from helpers import _tiny

LIB = os.path.join(PKG, "mgadmm", "libmgadmm.so")
NAMES = ["rho", "rho_u", "rho_d", "mu_u", "mu_d1", "mu_d2"]


def _header():
    txt = open(os.path.join(ROOT, "include", "mgadmm.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _symbols():
    if shutil.which("nm"):
        cmd = ["nm", "-C", LIB]
    else:
        cmd = [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump"), "--syms", "--demangle", LIB]
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def test_header_declares_the_struct_and_the_entry_point():
    h = _header()
    m = re.search(r"typedef struct \{([^{}]*)\} mgadmm_sample_params;", h)
    assert m, "mgadmm_sample_params is not declared"
    body = m.group(1)
    assert re.fullmatch(r"\s*const double\s*(\*\s*\w+\s*,\s*)*\*\s*\w+\s*;\s*", body), body      # six `const double*` and nothing else
    assert re.findall(r"\*\s*(\w+)", body) == NAMES
    assert re.search(r"int mgadmm_solver_set_sample_params\(mgadmm_solver\* s, const mgadmm_sample_params\* sp, int32_t B\);", h)


def test_binding_mirrors_the_header():
    from mgadmm import _lib
    assert [f[0] for f in _lib.SampleParams._fields_] == NAMES
    assert all(f[1] is C.POINTER(C.c_double) for f in _lib.SampleParams._fields_)
    assert C.sizeof(_lib.SampleParams) == 6 * C.sizeof(C.c_void_p)
    res, args = _lib.SYMBOLS["mgadmm_solver_set_sample_params"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(_lib.SampleParams), C.c_int32]
    assert _lib.lib.mgadmm_solver_set_sample_params.argtypes == args


def test_library_exports_the_symbol_and_a_null_solver_is_invalid():
    from mgadmm import _lib
    assert re.search(r"\bT mgadmm_solver_set_sample_params\b", _symbols()) or "mgadmm_solver_set_sample_params" in _symbols()
    assert _lib.lib.mgadmm_solver_set_sample_params(None, None, 0) == _lib.ERR_INVALID
    assert b"set_sample_params" in _lib.lib.mgadmm_last_error()


def test_version_counts_the_addition_and_no_struct_grew():
    from mgadmm import _lib
    m = re.match(r"mgadmm 0\.3\.(\d+) ", _lib.version())
    assert m and int(m.group(1)) >= 1, _lib.version()
    assert "0.3.1: mgadmm_solver_set_sample_params" in open(os.path.join(ROOT, "include", "mgadmm.h")).read()
    assert _lib.Params._fields_[-1][0] == "admm_convergence" and _lib.History._fields_[-1][0] == "n_iters_per_sample"


def test_one_pp_instance_per_default_instance():
    """The third translation unit compiles the instances of k_admm_lds again, as kernels of another name."""
    out = _symbols()
    base = set(re.findall(r"__device_stub__k_admm_lds(<[^>]*>)", out))
    pp = set(re.findall(r"__device_stub__k_admm_lds_pp(<[^>]*>)", out))
    ps = set(re.findall(r"__device_stub__k_admm_lds_ps(<[^>]*>)", out))
    assert len(base) == 45 and pp == base, dict(missing=sorted(base - pp), extra=sorted(pp - base))
    assert ps == base


BAD = [
    ({"rho_x": [1, 1, 1]}, "unknown key 'rho_x'"),
    ({"rho": [1, 1]}, "length B = 3"),
    ({"mu_u": [[1, 1, 1]]}, "length B = 3"),
    ({"mu_u": 1.0}, "length B = 3"),
    ({"rho": [1, 0, 1]}, r"\['rho'\]\[1\]"),
    ({"rho_u": torch.tensor([1.0, 1.0, -2.0])}, r"\['rho_u'\]\[2\]"),
    ({"rho_d": [0.0, 1, 1]}, r"\['rho_d'\]\[0\]"),
    ({"mu_d1": [1, float("nan"), 1]}, r"\['mu_d1'\]\[1\] is not finite"),
    ({"mu_d2": np.array([1, 1, np.inf])}, r"\['mu_d2'\]\[2\] is not finite"),
    ({"mu_u": [1, 1, -1e-9]}, r"\['mu_u'\]\[2\]"),
    ([1, 2, 3], "must be a dict"),
]


@pytest.mark.parametrize("sp, msg", BAD, ids=[m for _, m in BAD])
def test_sample_params_are_validated_before_the_library_is_touched(sp, msg, monkeypatch):
    """ValueError out of solve() and combined_loop() without a device: the check comes first (a solve on this machine
    would fail later, at the device, with another exception)."""
    blk = _tiny()
    touched = []
    monkeypatch.setattr(type(blk), "_solver", lambda self, *a: touched.append(a))
    y = torch.ones(3, 12, 2, 1)
    with pytest.raises(ValueError, match=msg):
        blk.solve(y, sample_params=sp)
    with pytest.raises(ValueError, match=msg):
        blk.combined_loop(y, print_info=False, sample_params=sp)
    assert touched == [] and blk._solvers == {}


def test_accepted_values():
    from mgadmm.ADMM import SAMPLE_PARAM_NAMES, _check_sample_params
    assert list(SAMPLE_PARAM_NAMES) == NAMES
    out = _check_sample_params({"mu_u": [0, 1, 2], "rho": torch.tensor([1, 2, 3])}, 3)        # mu = 0 is allowed, ints are
    assert list(out) == ["mu_u", "rho"]
    assert all(v.dtype == np.float64 and v.flags.c_contiguous and v.shape == (3,) for v in out.values())
    assert out["rho"].tolist() == [1.0, 2.0, 3.0] and out["mu_u"].tolist() == [0.0, 1.0, 2.0]
    assert _check_sample_params({}, 3) == {}


class _Stub:
    """solve() of an instance replaced: records what sweep() asks for and answers with tensors that name the sample."""

    def __init__(self, blk):
        self.blk, self.calls = blk, []

    def __call__(self, y, mask=None, sample_params=None, **kw):
        self.calls.append(dict(y=y.clone(), mask=None if mask is None else mask.clone(), sp=sample_params, kw=kw))
        B = y.shape[0]
        code = torch.tensor([100 * sample_params["mu_u"][b] + 10 * sample_params["mu_d1"][b] for b in range(B)])
        x = (y[:, :1, :1, :1] + code.reshape(B, 1, 1, 1)).expand(B, 24, 2, 1).clone()
        self.blk.n_iters_per_sample = (y[:, 0, 0, 0] + code).numpy().astype(np.int32)
        return x, (None, None), None, {}


def test_sweep_forms_the_product_with_the_window_index_fastest(monkeypatch):
    blk = _tiny()
    stub = _Stub(blk)
    monkeypatch.setattr(blk, "solve", stub)
    W = 4
    y = torch.arange(W, dtype=torch.float32).reshape(W, 1, 1, 1).expand(W, 12, 2, 1).clone()       # window w holds the value w
    grid = {"mu_u": [0.5, 1, 2], "mu_d1": [1, 2]}
    x, n, sets = blk.sweep(y, grid, per_sample_history=True)
    assert sets == [dict(mu_u=a, mu_d1=b) for a in (0.5, 1, 2) for b in (1, 2)]                    # itertools.product order
    assert tuple(x.shape) == (6, W, 24, 2, 1) and n.shape == (6, W) and n.dtype == np.int32
    assert len(stub.calls) == 1 and stub.calls[0]["y"].shape[0] == 6 * W
    c = stub.calls[0]
    assert c["kw"] == {"per_sample_history": True, "return_state": False} and c["mask"] is None
    assert list(c["sp"]) == ["mu_u", "mu_d1"] and all(len(v) == 6 * W for v in c["sp"].values())
    for p, s in enumerate(sets):
        for w in range(W):
            want = w + 100 * s["mu_u"] + 10 * s["mu_d1"]
            assert float(x[p, w, 0, 0, 0]) == want and n[p, w] == int(want), (p, w)
            assert c["sp"]["mu_u"][p * W + w] == s["mu_u"] and float(c["y"][p * W + w, 0, 0, 0]) == w
    # in pieces: the same tensors from consecutive slices of the same batch (the last piece is shorter)
    stub.calls.clear()
    mask = torch.ones(W, 12, 2, 1)
    x2, n2, sets2 = blk.sweep(y, grid, mask=mask, chunk=10)
    assert [c["y"].shape[0] for c in stub.calls] == [10, 10, 4] and all(c["mask"].shape[0] == c["y"].shape[0] for c in stub.calls)
    assert torch.equal(x2, x) and np.array_equal(n2, n) and sets2 == sets
    with pytest.raises(ValueError, match="unknown key"):
        blk.sweep(y, {"sigma": [1]})
    with pytest.raises(ValueError, match="chunk"):
        blk.sweep(y, grid, chunk=0)
