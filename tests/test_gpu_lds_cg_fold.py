"""p . A p from q . q in the cLdr solves of the uniform-row k_admm_lds instances (csrc/lds_kernels.h, lds_apply FOLD: three
barriers per CG iteration instead of four) against the generic instance of the same library and the float64 oracle.

MGADMM_LDS_RAGGED=1 plans the generic instance (tables in LDS, p . A p summed after the W_d^T gather) for a graph whose rows
qualify for a uniform one; MGADMM_LDS_TPG pins both legs to the same time-group width.  The switches are read when a solver is
planned, so each leg runs in a child process (`python tests/lds_cg_fold_cases.py <case> <out.npz>`).  Per case:
  * the plan: the default leg runs the uniform instance and MGADMM_Q_LDS_CG_BARRIERS says 3, the ragged leg the generic
    instance and 4;
  * either leg against the float64 oracle on windows 0, B // 2, B - 1 through helpers.check_windows at the tolerances of the
    BASELINE configs (x per sample 1e-5, history lists rtol 1e-3, CG counts +-1), exported zu / phi at 1e-4 / 1e-3;
  * the legs against each other at the bounds of test_gpu_lds_row_order.py: x per sample within 2e-5 (two float32 results
    that are each within 1e-5 of the oracle), the exported state within 2e-4, CG counts within 2.
Cases: the bench's cfg2 graph at B = 96 with 16 iterations in one launch; masked input (cfg2 under 'DGTV', the N = 128 graph
under 'None'); the three ablations; a TPG 12 case; hub graphs with tail pairs 0 to 3.  On the golden k = 4 tables: a
sample_params batch (k_admm_lds_pp), a per-sample-stop batch (k_admm_lds_ps) whose samples still equal their B = 1 solves bit
for bit, and the same table with use_kNN=False (transpose by gather, quirk Q4: p . A p is not the q form there,
tests/test_cg_fold_cpu.py), which must get a generic instance.
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import lds_cg_fold_cases as fc
import lds_row_order_cases as rc
from lds_row_order_cases import LISTS

pytestmark = pytest.mark.gpu

ZU_TOL, PHI_TOL = 1e-4, 1e-3           # test_gpu_parity.py: float32 zu / phi against the float64 reference
X_PAIR_TOL, STATE_PAIR_TOL, CG_PAIR = 2e-5, 2e-4, 2


def _leg(name, tmp_path, ragged, tpg=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MGADMM_LDS_")}
    if ragged:
        env["MGADMM_LDS_RAGGED"] = "1"
    if tpg is not None:
        env["MGADMM_LDS_TPG"] = str(tpg)
    out = str(tmp_path / f"{name}_{int(ragged)}.npz")
    p = subprocess.run([sys.executable, "-s", fc.__file__, name, out], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return dict(np.load(out))


def _per_sample_rel(a, b):
    a = a.reshape(a.shape[0], -1).astype(np.float64)
    b = b.reshape(b.shape[0], -1).astype(np.float64)
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


def _as_blk(d, prefix=""):
    return types.SimpleNamespace(metrics_per_sample=d[prefix + "mps"], **{k: [torch.from_numpy(v) for v in d[prefix + k]] for k in LISTS})


def _exported_state_against(tag, d, o, idx):
    for k, tol in (("zu", ZU_TOL), ("phi", PHI_TOL)):
        if k in o.state and "state_" + k in d:
            e = np.linalg.norm(d["state_" + k][idx].astype(np.float64) - o.state[k]) / np.linalg.norm(o.state[k])
            print(f"[cg fold] {tag}: exported {k} against the oracle {e:.2e}")
            assert e <= tol, (tag, k, e)


def _graph_oracle(c, y, mask, idx):
    """The float64 oracle on windows idx of a graph case (weight tables as the product builds them)."""
    import mgadmm
    from oracle import admm_oracle as orc
    kw = dict(u_sigma=c["sigma"], d_sigma=c["sigma"]) if c["sigma"] else {}
    ref = mgadmm.ADMM_algorithm({"n_nodes": c["N"]}, c["info"], use_kNN=True, k=4, tables=c["tables"], ablation=c["abl"],
                                t_in=c["t_in"], T=c["T"], record_cg_coeffs=False, path="stream", **kw)
    o = orc.OracleADMM(ref.connect_list.numpy(), ref.u_ew[0].numpy(), ref.d_ew[0].numpy(), c["info"], mode="knn", ablation=c["abl"],
                       t_in=c["t_in"], T=c["T"])
    ref.close()
    xo = o.combined_loop(y[idx].astype(np.float64), mask=None if mask is None else mask[idx], n_iters=c["iters"])
    return o, xo


def _assert_pair(name, new, old):
    ex = _per_sample_rel(new["x"], old["x"])
    print(f"\n[cg fold] {name}: x per sample, uniform against generic: max {ex.max():.2e} median {np.median(ex):.2e}")
    assert ex.max() <= X_PAIR_TOL, (name, ex.max())
    for k in sorted(k for k in new if k.startswith("state_")):
        e = _per_sample_rel(new[k], old[k]).max()
        print(f"[cg fold] {name}: {k} {e:.2e}")
        assert e <= STATE_PAIR_TOL, (name, k, e)
    for k in LISTS:
        assert new[k].shape == old[k].shape, (name, k)
        if new[k].size:
            dcg = np.abs(new[k].astype(np.int64) - old[k].astype(np.int64)).max()
            print(f"[cg fold] {name}: {k} counts differ by at most {dcg}")
            assert dcg <= CG_PAIR, (name, k, dcg)


def _assert_plans(name, new, old, expect, ragged):
    """expect: the uniform instance's name, or its beginning (the golden graph: whatever tail its in-degrees need)"""
    assert str(new["instance"]).startswith(expect) and int(new["uniform"]) == 1 and int(new["barriers"]) == 3, (name, new["instance"], new["barriers"])
    assert str(old["instance"]) == ragged and int(old["uniform"]) == 0 and int(old["barriers"]) == 4, (name, old["instance"], old["barriers"])


G4_UNIFORM, G4_GENERIC = "k_admm_lds<8, false, 1024, false, 4, 5, ", "k_admm_lds<8, false, 1024, false, 0, 0, false, -1>"


@pytest.mark.parametrize("name", fc.GRAPH_CASES)
def test_uniform_instance_against_generic_instance_and_the_oracle(name, tmp_path):
    from helpers import check_windows
    c = fc.case(name)
    tpg = 12 if name == "tpg12" else 8
    y, mask = rc.inputs(c)
    new = _leg(name, tmp_path, False)
    old = _leg(name, tmp_path, True, tpg)
    _assert_plans(name, new, old, c["expect"], c["ragged"])
    B = c["B"]
    idx = np.array([0, B // 2, B - 1])
    o, xo = _graph_oracle(c, y, mask, idx)
    for tag, d in ((f"{name} uniform", new), (f"{name} generic", old)):
        check_windows(tag, _as_blk(d), torch.from_numpy(d["x"]), idx, o, xo, abl=c["abl"], finite_termination_rule=True)
        _exported_state_against(tag, d, o, idx)
    _assert_pair(name, new, old)
    if name == "cfg2":
        assert not np.array_equal(new["x"], old["x"])            # the switch reaches the planner: another summation order


def _oracle_with_row(meta, y64, b, table):
    from helpers import make_oracle
    o = make_oracle(meta, "knn")
    for nm in fc.PP_NAMES:
        setattr(o, nm, float(table[nm][b]))
    return o, o.combined_loop(y64[b:b + 1], n_iters=fc.PP_ITERS)


def test_sample_params_batch(tmp_path):
    """k_admm_lds_pp: every sample under its own weights, uniform against generic and either against the oracle built with the row."""
    from helpers import check_windows
    meta = fc.g4_meta()
    new = _leg("pp", tmp_path, False)
    old = _leg("pp", tmp_path, True, 8)
    _assert_plans("pp", new, old, G4_UNIFORM, G4_GENERIC)
    y64, table = fc.g5_y().astype(np.float64), fc.pp_table(meta)
    for b in (0, 3, 7):
        o, xo = _oracle_with_row(meta, y64, b, table)
        for tag, d in ((f"pp uniform sample {b}", new), (f"pp generic sample {b}", old)):
            check_windows(tag, _as_blk(d), torch.from_numpy(d["x"]), [b], o, xo)
    _assert_pair("pp", new, old)


def test_per_sample_stop_batch_equals_single_solves_bit_for_bit(tmp_path):
    """k_admm_lds_ps: samples stop on their own residuals; each still equals its B = 1 solve bit for bit (one workgroup owns one
    sample whatever the batch around it is), in either leg."""
    new = _leg("ps", tmp_path, False)
    old = _leg("ps", tmp_path, True, 8)
    _assert_plans("ps", new, old, G4_UNIFORM, G4_GENERIC)
    print("[cg fold] ps: iterations per sample, uniform", new["n"].tolist(), "generic", old["n"].tolist())
    assert new["n"].max() - new["n"].min() >= 10            # the samples do stop at different iterations
    for tag, d in (("uniform", new), ("generic", old)):
        for b in fc.PS_SINGLES:
            nb = int(d["n"][b])
            assert nb == int(d[f"single{b}_n"]), (tag, b)
            np.testing.assert_array_equal(d["x"][b], d[f"single{b}_x"][0], err_msg=f"{tag} {b}")
            np.testing.assert_array_equal(d["mps"][:nb, :, b], d[f"single{b}_mps"][:, :, 0], err_msg=f"{tag} {b}")
            for k in (k for k in d if k.startswith("state_")):
                np.testing.assert_array_equal(d[k][b], d[f"single{b}_{k}"][0], err_msg=f"{tag} {b} {k}")
            for k in LISTS:
                np.testing.assert_array_equal(d[k][:nb, b], d[f"single{b}_{k}"][:, 0], err_msg=f"{tag} {b} {k}")
    # the legs against each other: each stop iteration is within 1 of the oracle's (test_gpu_admm_per_sample.py), so within 2 here;
    # samples that stop at the same iteration compare like any two float32 results
    assert np.abs(new["n"].astype(np.int64) - old["n"].astype(np.int64)).max() <= 2
    same = new["n"] == old["n"]
    if same.any():
        ex = _per_sample_rel(new["x"][same], old["x"][same])
        print(f"[cg fold] ps: x per sample ({int(same.sum())} of 8 samples stop at the same iteration in both legs): max {ex.max():.2e}")
        assert ex.max() <= X_PAIR_TOL


def test_transpose_by_gather_never_gets_a_uniform_instance(tmp_path):
    """use_kNN=False on a k = 4 table without pads: rows of 4 and 5 entries, but the second operator gathers with W_d itself."""
    from helpers import check_windows
    d = _leg("physical", tmp_path, False)
    assert int(d["uniform"]) == 0 and int(d["barriers"]) == 4, (d["uniform"], d["barriers"])
    inst = str(d["instance"])
    assert ", 0, 0, false, -1>" in inst and ", 4, 5," not in inst, inst
    meta = fc.g4_meta(physical_on_knn_tables=True)
    y64 = fc.g5_y().astype(np.float64)
    idx = np.array([0, 4, 7])
    from helpers import make_oracle
    o = make_oracle(meta, "physical")
    xo = o.combined_loop(y64[idx], n_iters=fc.PP_ITERS)
    check_windows("physical on the kNN table", _as_blk(d), torch.from_numpy(d["x"]), idx, o, xo)
    _exported_state_against("physical on the kNN table", d, o, idx)
