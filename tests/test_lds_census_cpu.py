"""CPU checks of the k_admm_lds instance census (tests/lds_census.py): the census covers exactly the instances the built
library ships, and the census graphs have the W_d^T in-degrees their rows state."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import lds_census as lc
from conftest import PKG

LIB = os.path.join(PKG, "mgadmm", "libmgadmm.so")


def shipped_instances():
    """Names of the k_admm_lds instances compiled into the library (one host launch stub per instance)."""
    if shutil.which("nm"):
        cmd = ["nm", "-C", LIB]
    else:
        cmd = [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump"), "--syms", "--demangle", LIB]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    return set(re.findall(r"__device_stub__(k_admm_lds<[^>]*>)", out))


def test_census_covers_every_shipped_instance():
    shipped = shipped_instances()
    census = [r["expect"] for r in lc.CENSUS]
    assert len(census) == len(set(census)), "two census rows for one instance"
    assert len(shipped) == 45, sorted(shipped)
    assert set(census) == shipped, dict(missing=sorted(shipped - set(census)), stale=sorted(set(census) - shipped))


def test_instance_decoder():
    from mgadmm import _lib
    assert _lib.decode_lds_instance(-1) is None
    v = 12 | 1 << 10 | 4 << 11 | 5 << 16 | 640 << 21 | (2 + 1) << 32
    assert _lib.decode_lds_instance(v) == "k_admm_lds<12, false, 640, false, 4, 5, true, 2>"
    v = 8 | 1 << 8 | 1 << 9 | 1024 << 21
    assert _lib.decode_lds_instance(v) == "k_admm_lds<8, true, 1024, true, 0, 0, false, -1>"
    assert _lib.Q_LDS_INSTANCE == 16


def _check_table(cl, dl):
    cl, dl = cl.numpy(), dl.numpy()
    N = cl.shape[0]
    assert (cl[:, 0] == np.arange(N)).all() and (dl[:, 0] == 0).all()
    for i in range(N):
        nb = cl[i, 1:][cl[i, 1:] != -1]
        assert len(set(nb.tolist())) == len(nb) and i not in nb and ((nb >= 0) & (nb < N)).all()
        d = dl[i, 1:][cl[i, 1:] != -1]
        assert (d > 0).all() and (np.diff(d) > 0).all()


@pytest.mark.parametrize("r", [r for r in lc.CENSUS if r["kind"] == "uniform"], ids=lc.row_id)
def test_uniform_tables_have_the_stated_in_degree(r):
    cl, dl = lc.tables_for(r)
    assert tuple(cl.shape) == tuple(dl.shape) == (r["N"], 5) and cl.dtype == torch.int64 and dl.dtype == torch.float32
    assert (cl != -1).all()
    _check_table(cl, dl)
    deg = lc.in_degrees(cl.numpy())
    assert deg.max() == r["indeg"] and deg[0] == r["indeg"]           # node 0 is the hub
    assert (deg == 0).any()                                             # a W_d^T row of padding only
    assert (deg == r["indeg"]).sum() == (1 if r["indeg"] > 5 else 4)    # one hub (in-degree 5: three helpers beside it)
    tp = lc.tail_pairs(r["indeg"])
    m = re.match(r"k_admm_lds<.*, (-?\d+)>$", r["expect"])
    if r["env"].get("MGADMM_LDS_SB"):
        assert int(m.group(1)) == -1
    else:
        assert int(m.group(1)) == (tp if tp <= 3 else -1), (tp, r["expect"])


def test_in_degrees_of_the_generator_cover_every_tail_form():
    """5, 6, 7, 9, 11, 12 and a long run-time tail: TP 0, both parities of TP 1, TP 2, TP 3, the first run-time count."""
    degs = {r["indeg"] for r in lc.CENSUS if r["kind"] == "uniform"}
    assert {5, 6, 7, 9, 11, 12} <= degs and max(degs) >= 25
    assert [lc.tail_pairs(d) for d in (5, 6, 7, 9, 11, 12, 25)] == [0, 1, 1, 2, 3, 4, 10]


@pytest.mark.parametrize("kind", ["knn3", "knnpad", "line1"])
def test_ragged_tables(kind):
    r = next(r for r in lc.CENSUS if r["kind"] == kind)
    cl, dl = lc.tables_for(r)
    _check_table(cl, dl)
    lens = (cl[:, 1:] != -1).sum(1).numpy()
    deg = lc.in_degrees(cl.numpy())
    if kind == "knn3":
        assert cl.shape[1] == 4 and (lens == 3).all()
    elif kind == "knnpad":
        assert (lens[-3:] == 2).all() and (lens[:-3] == 4).all()          # -1 pads in the small component's rows
        assert deg[-3:].tolist() == [2, 2, 2]
    else:
        assert (lens == 4).all()


def test_physical_graph_has_ragged_rows():
    from mgadmm import utils
    r = next(r for r in lc.CENSUS if r["kind"] == "physical" and r["N"] == 307)
    ue, ud = lc.physical_graph(r["N"])
    cl, _ = utils.connect_list(r["N"], ue, ud)
    lens = (np.asarray(cl)[:, 1:] != -1).sum(1)
    assert lens.min() <= 2 and lens.max() >= 8
    assert len(set(lens[:64].tolist())) >= 3                           # lengths vary within the first wave


def test_census_geometry_covers_the_edges():
    """The rows' planner geometry (asserted on the GPU): ghost threads 0, 1 and 63, time groups 1, 2, 3, 4 and 6, and the
    unpadded row stride TS = T."""
    assert set(lc.GEOMETRY) == {r["expect"][len("k_admm_lds"):] for r in lc.CENSUS}
    geo = [lc.geometry(r) for r in lc.CENSUS]
    assert {0, 1, 63} <= {g[3] for g in geo}
    assert {1, 2, 3, 4, 6} <= {lc.GEOMETRY[r["expect"][len("k_admm_lds"):]][0] for r in lc.CENSUS}
    padded = lambda T: (T + 3) // 4 * 4 + (4 if (((T + 3) // 4) & 1) == 0 else 0)
    assert any(g[2] == r["T"] != padded(r["T"]) for r, g in zip(lc.CENSUS, geo))
    for r, (nth, rows, ts, ghosts) in zip(lc.CENSUS, geo):
        tpg = int(re.match(r"k_admm_lds<(\d+),", r["expect"]).group(1))
        assert r["T"] % tpg == 0 and nth == r["N"] * (r["T"] // tpg) <= 1024 and ts >= r["T"]
