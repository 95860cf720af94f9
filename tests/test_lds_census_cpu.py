"""CPU checks of the k_admm_lds instance census (tests/lds_census.py): the census covers exactly the instances the built
library ships -- in each of its three compilations (k_admm_lds, k_admm_lds_ps, k_admm_lds_pp) --, the census graphs have the
W_d^T in-degrees their rows state, and the tolerance picker of tests/test_gpu_lds_census_units.py keeps its conditions."""
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


def shipped_instances(kernel="k_admm_lds"):
    """Names of the instances of `kernel` compiled into the library (one host launch stub per instance)."""
    if shutil.which("nm"):
        cmd = ["nm", "-C", LIB]
    else:
        cmd = [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump"), "--syms", "--demangle", LIB]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    return set(re.findall(r"__device_stub__(" + kernel + r"<[^>]*>)", out))


def test_census_covers_every_shipped_instance():
    shipped = shipped_instances()
    census = [r["expect"] for r in lc.CENSUS]
    assert len(census) == len(set(census)), "two census rows for one instance"
    assert len(shipped) == 45, sorted(shipped)
    assert set(census) == shipped, dict(missing=sorted(shipped - set(census)), stale=sorted(set(census) - shipped))


@pytest.mark.parametrize("kernel", ["k_admm_lds_ps", "k_admm_lds_pp"])
def test_the_other_two_compilations_ship_the_same_instances(kernel):
    """lds_launch_ps.hip and lds_launch_pp.hip: 45 instances each, with the argument lists of the 45 k_admm_lds instances and
    of the census rows (tests/test_gpu_lds_census_units.py launches every one of them)."""
    args = lambda names, k: sorted(n[len(k):] for n in names)
    shipped = shipped_instances(kernel)
    assert len(shipped) == 45 and all(n.startswith(kernel + "<") for n in shipped), sorted(shipped)
    assert args(shipped, kernel) == args(shipped_instances(), "k_admm_lds")
    assert args(shipped, kernel) == args([r["expect"] for r in lc.CENSUS], "k_admm_lds")


def test_unit_query_is_declared():
    from mgadmm import _lib
    assert _lib.Q_LDS_UNIT == 18 and _lib.Q_LDS_CG_BARRIERS == 17 and _lib.Q_LDS_INSTANCE == 16
    assert _lib.LDS_UNITS == ("k_admm_lds", "k_admm_lds_ps", "k_admm_lds_pp")
    header = open(os.path.join(os.path.dirname(PKG), "include", "mgadmm.h")).read()
    assert re.search(r"MGADMM_Q_LDS_UNIT = 18\b", header)


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


# ------------------------------------------------------------------------------- the tolerance picker of the unit census
def _decay(first, factor, K=12):
    return first * factor ** np.arange(K)


def test_picker_on_a_monotone_table():
    """Three geometric decays a factor 2 and 4 apart: the picks stop at different iterations in different launches."""
    res = np.stack([_decay(100.0, 0.8), _decay(200.0, 0.8), _decay(400.0, 0.8)])
    tol, n = lc.pick_admm_tol(res, 12)
    assert n == lc.stop_iterations(res, tol, 12)
    for row, v in zip(res, n):
        assert (row[:v - 1] >= tol).all() and row[v - 1] < tol                  # n_b is the first crossing
        assert (np.abs(row[:v] / tol - 1) > lc.UNIT_MARGIN).all()
    assert all(2 <= v <= 11 for v in n) and len(set(n)) == 3 and n == sorted(n)
    assert len({-(-v // lc.UNIT_CHUNK) for v in n}) == 3                         # the most launches the table allows
    # the factor 0.8 puts 100 * 0.8^k, 200 * 0.8^(k+3.1), 400 * 0.8^(k+6.2) apart: the gap to the nearest residual is > 1 %
    assert min(np.abs(np.log(res / tol)).min(), 1.0) > np.log(1.01)


def test_picker_on_a_table_with_a_bump():
    """The second residual is larger than the first (the census rows with a phi update look like this): a tolerance between
    the two would stop a pick at iteration 1 although its residual comes back above it.  n_b is the FIRST crossing, so such a
    tolerance breaks the [2, K - 1] condition and the picker goes below the first residual."""
    base = np.array([76.0, 90.7, 45.3, 41.3, 38.7, 36.3, 34.1, 32.1, 30.1, 28.3, 26.6, 25.1])
    res = np.stack([base, 1.5 * base, 2.0 * base])
    tol, n = lc.pick_admm_tol(res, 12)
    assert tol < base[0] and n[0] >= 3
    assert all((row[:v - 1] >= tol).all() and row[v - 1] < tol for row, v in zip(res, n))
    assert len({-(-v // 4) for v in n}) >= 2
    with pytest.raises(AssertionError, match=r"not all in \[2, 11\]"):
        lc.stop_iterations(res, 80.0, 12)                                        # pick 0 would stop at iteration 1
    # a bump back over the tolerance AFTER the first crossing does not move n_b
    late = res.copy()
    late[0, n[0]] = 10 * tol
    assert lc.stop_iterations(late, tol, 12) == n


def test_picker_raises_on_a_table_that_cannot_meet_the_conditions():
    flat = np.stack([_decay(100.0, 0.99), _decay(200.0, 0.99), _decay(400.0, 0.99)])       # nobody reaches another's level
    with pytest.raises(AssertionError, match="no tolerance meets"):
        lc.pick_admm_tol(flat, 12)
    same = np.stack([_decay(100.0, 0.8)] * 3)                                              # every pick stops at the same iteration
    with pytest.raises(AssertionError, match="no tolerance meets"):
        lc.pick_admm_tol(same, 12)
    # three halvings, then a plateau: the picks cross at 3 / 4 in the first launch, or one of them never does
    one_launch = np.stack([np.concatenate([_decay(f, 0.5, 4), _decay(f / 8, 0.9999, 9)[1:]]) for f in (100.0, 110.0, 120.0)])
    with pytest.raises(AssertionError, match="no tolerance meets"):
        lc.pick_admm_tol(one_launch, 12)
    ok = np.stack([_decay(100.0, 0.8), _decay(200.0, 0.8), _decay(400.0, 0.8)])
    with pytest.raises(AssertionError, match="within 0.01"):                               # a stop on a rounding decision
        lc.stop_iterations(ok, ok[0, 3] * 1.005, 12)
    with pytest.raises(AssertionError, match="never falls below"):
        lc.stop_iterations(ok, 1.0, 12)
    with pytest.raises(AssertionError, match="same launch"):
        lc.stop_iterations(ok[:1] * np.array([[1.0], [1.15]]), 70.0, 12)                   # iterations 3 and 4: the first launch


def test_unit_census_overrides_name_census_rows():
    rows = {r["expect"]: r for r in lc.CENSUS}
    for k, v in lc.UNIT_OVERRIDES.items():
        assert k in rows and set(v) <= {"K", "scales"}, k
        assert v.get("K", lc.UNIT_K) <= 24
        if "scales" in v:
            assert len(v["scales"]) == rows[k]["B"] and len(set(np.asarray(v["scales"])[lc.unit_picks(rows[k])])) == 3
    for r in lc.CENSUS:
        s = lc.unit_scales(r)
        assert s.shape == (r["B"],) and (np.diff(s) > 0).all() and s[0] >= 0.5 and s[-1] <= 2.0
        assert len(set(lc.unit_picks(r))) == 3
