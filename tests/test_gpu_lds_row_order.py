"""k_admm_lds with its rows owned long-W_d^T-rows-first (csrc/lds_rows.h: the default of the uniform-row instances with a
compile-time tail is the order by tail pairs needed; MGADMM_LDS_ROW_ORDER=1 is the order by in-degree) against the same
library in node order (MGADMM_LDS_ROW_ORDER=0) and against the float64 oracle.

The switch is read when a solver is planned, so each setting runs in a child process of its own
(`python tests/lds_row_order_cases.py <case> <out.npz>`), which solves the case and writes x, the exported state, the
per-sample metric sums and the CG counts.  The parent compares:
  * either leg with the float64 oracle on windows 0, B // 2, B - 1 at the tolerances of the BASELINE configs
    (helpers.check_windows: x per sample 1e-5, history lists rtol 1e-3, CG counts +-1), and the exported zu / phi at the
    bounds of test_gpu_parity.py (1e-4 / 1e-3) -- the exported state passes through k_state_layout with row_of_node, a wrong
    map there is an O(1) error;
  * the two legs with each other: x per sample within 2e-5 (two float32 results that are each within 1e-5 of the oracle), the
    other exported vectors within 2e-4 (the census bound of 1e-4 for each), CG counts within 2;
  * the same instance ran in both legs.
EVERY case runs three settings: node order, the default order and the in-degree order.  The hub graphs of the census hold
their only row of in-degree > 5 at node 0, so the default order (by tail pairs needed) leaves them in node order -- there the
default leg tests the per-wave counts alone, and the in-degree leg is the one that meets a permutation (258 of 341, 33 of 43,
50 of 100, 75 of 150, 64 of 128 rows move).  The default order permutes the bench graph (cfg2, cfg2mask: 49 rows of in-degree
> 5 move to the front).  The test asserts, per case and leg, that the permutation it claims to cover is not the identity
(`rows_moved`, held against the C++ plan by tests/test_lds_rows_cpu.py).
Cases: the bench's cfg2 graph at B = 96 with 16 iterations in one launch, and with masked input under 'DGTV'; hub graphs
with tail_pairs 0, 1, 2 and 3 (census
rows: 1 ghost / 63 ghosts in a last wave that is mostly ghosts / G = 6), a graph where no wave straddles two time groups
(N = 128), masked input, the three ablations; and a warm start from an exported state: k1 + k2 iterations in two calls equal
k1 + k2 in one, bit for bit (the state makes the round trip through k_state_layout in row order).
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import lds_row_order_cases as rc
from lds_row_order_cases import LISTS

pytestmark = pytest.mark.gpu

ZU_TOL, PHI_TOL = 1e-4, 1e-3           # test_gpu_parity.py: float32 zu / phi against the float64 reference
X_PAIR_TOL, STATE_PAIR_TOL = 2e-5, 2e-4
SETTINGS = {"node order": "0", "default order": None, "in-degree order": "1"}
PERMUTED_BY_DEFAULT = ("cfg2", "cfg2mask")


def _leg(name, tmp_path, row_order):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MGADMM_LDS_")}
    if row_order is not None:
        env["MGADMM_LDS_ROW_ORDER"] = row_order
    out = str(tmp_path / f"{name}_{row_order}.npz")
    p = subprocess.run([sys.executable, "-s", rc.__file__, name, out], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return dict(np.load(out))


def _assert_permuted(name, c, leg):
    """The leg meets a permutation where the test claims it does: in-degree order on every case, the default on the bench graph."""
    moved = rc.rows_moved(c["tables"][0].numpy(), rc.IN_DEGREE if leg == "in-degree order" else rc.TAIL_CLASS)
    print(f"[row order] {name} {leg}: {moved} of {c['N']} rows are another node than in node order")
    if leg == "in-degree order" or name in PERMUTED_BY_DEFAULT:
        assert moved >= c["N"] // 8, (name, leg, moved)
    return moved


def _per_sample_rel(a, b):
    a = a.reshape(a.shape[0], -1).astype(np.float64)
    b = b.reshape(b.shape[0], -1).astype(np.float64)
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


def _against_oracle(tag, c, d, y, mask):
    from helpers import check_windows
    from oracle import admm_oracle as orc
    import mgadmm
    B = c["B"]
    idx = np.array([0, B // 2, B - 1])
    kw = dict(u_sigma=c["sigma"], d_sigma=c["sigma"]) if c["sigma"] else {}
    ref = mgadmm.ADMM_algorithm({"n_nodes": c["N"]}, c["info"], use_kNN=True, k=4, tables=c["tables"], ablation=c["abl"],
                                t_in=c["t_in"], T=c["T"], record_cg_coeffs=False, path="stream", **kw)    # (the weight tables)
    o = orc.OracleADMM(ref.connect_list.numpy(), ref.u_ew[0].numpy(), ref.d_ew[0].numpy(), c["info"], mode="knn", ablation=c["abl"],
                       t_in=c["t_in"], T=c["T"])
    ref.close()
    xo = o.combined_loop(y[idx].astype(np.float64), mask=None if mask is None else mask[idx], n_iters=c["iters"])
    blk = types.SimpleNamespace(metrics_per_sample=d["mps"], **{k: [torch.from_numpy(v) for v in d[k]] for k in LISTS})
    check_windows(tag, blk, torch.from_numpy(d["x"]), idx, o, xo, abl=c["abl"], finite_termination_rule=True)
    for k, tol in (("zu", ZU_TOL), ("phi", PHI_TOL)):
        if k in o.state and "state_" + k in d:
            e = np.linalg.norm(d["state_" + k][idx].astype(np.float64) - o.state[k]) / np.linalg.norm(o.state[k])
            print(f"[row order] {tag}: exported {k} against the oracle {e:.2e}")
            assert e <= tol, (tag, k, e)


@pytest.mark.parametrize("name", ["cfg2", "cfg2mask", "hub0", "hub1", "hub2", "hub3", "aligned"])
def test_row_order_against_node_order_and_the_oracle(name, tmp_path):
    c = rc.case(name)
    y, mask = rc.inputs(c)
    old = _leg(name, tmp_path, SETTINGS["node order"])
    assert str(old["instance"]) == c["expect"]
    _against_oracle(f"{name} node order", c, old, y, mask)
    for leg in ("default order", "in-degree order"):
        moved = _assert_permuted(name, c, leg)
        new = _leg(name, tmp_path, SETTINGS[leg])
        assert str(new["instance"]) == c["expect"]
        ex = _per_sample_rel(new["x"], old["x"])
        print(f"\n[row order] {name}: x per sample, {leg} against node order: max {ex.max():.2e} median {np.median(ex):.2e}")
        _against_oracle(f"{name} {leg}", c, new, y, mask)
        assert ex.max() <= X_PAIR_TOL, (name, leg, ex.max())
        for k in sorted(k for k in new if k.startswith("state_")):
            e = _per_sample_rel(new[k], old[k]).max()
            print(f"[row order] {name} {leg}: {k} {e:.2e}")
            assert e <= STATE_PAIR_TOL, (name, leg, k, e)
        for k in LISTS:
            assert new[k].shape == old[k].shape
            if new[k].size:
                assert np.abs(new[k].astype(np.int64) - old[k].astype(np.int64)).max() <= 2, (name, leg, k)
        if moved and name.startswith("cfg2"):
            assert not np.array_equal(new["x"], old["x"])            # the switch reaches the planner: other summation order


def test_resume_through_the_exported_state_is_bitwise(tmp_path):
    """Every setting: the resumed solve equals the uninterrupted one bit for bit, and the result is the oracle's (the in-degree
    leg is the one whose state makes the round trip through k_state_layout under a permutation: 64 of 128 rows move)."""
    c = rc.case("resume")
    y, mask = rc.inputs(c)
    for leg, order in SETTINGS.items():
        if leg != "node order":
            _assert_permuted("resume", c, leg)
        d = _leg("resume", tmp_path, order)
        assert str(d["instance"]) == c["expect"]
        np.testing.assert_array_equal(d["x_resumed"], d["x"])
        np.testing.assert_array_equal(np.concatenate([d["mps_first"], d["mps_second"]]), d["mps"])
        for k in (k for k in d if k.startswith("state_")):
            np.testing.assert_array_equal(d["resumed_" + k], d[k], err_msg=k)
        _against_oracle(f"resume {leg}", c, d, y, mask)
