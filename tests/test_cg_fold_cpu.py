"""Where k_admm_lds may take p . A p from q . q (csrc/lds_kernels.h, lds_apply FOLD).

The cLdr systems are A = diag(dc) + c2 Ldr^T Ldr (LHS_x: dc = [t < t_in] + (rho_u + rho_d) / 2, c2 = rho / 2; LHS_zd:
dc = rho_d / 2, c2 = mu_d2), so p . A p = sum dc p^2 + c2 |Ldr p|^2 -- as long as the operator applied second is the exact
transpose of Ldr.  On the float64 oracle:
  * kNN and line / skip graphs, with the reference's quirks on and off (Q1 adds the identity on the t = 0 block of Ldr^T, where
    Ldr p is zero): the two sides agree to 1e-12 relative;
  * mode="physical" (use_kNN=False, quirk Q4: the second operator gathers with W_d itself) on an unpadded k = 4 table: they do
    NOT agree, so the planner (csrc/lds_plan.h) must never give such a graph a uniform-row (folded) instance:
    tests/test_lds_plan_cpu.py asserts that on the planner itself, tests/test_gpu_lds_cg_fold.py on the GPU.
"""
import numpy as np
import pytest

from conftest import admm_info_from
from oracle import admm_oracle as orc

REL = 1e-12


def _oracle(meta, mode, bug_compat):
    info = admm_info_from(meta)
    T, t_in = int(meta["T"]), int(meta["t_in"])
    if mode in ("line", "skip3"):
        return orc.OracleADMM(meta["knn_cl"], meta["knn_u_ew"], None, info, mode="line", t_in=t_in, T=T,
                              skip_connection=1 if mode == "line" else 3, bug_compat=bug_compat)
    # 'physical' on the kNN table: k = 4, no pads -- the table shape that qualifies for the uniform-row instances
    return orc.OracleADMM(meta["knn_cl"], meta["knn_u_ew"], meta["knn_d_ew"], info, mode=mode, t_in=t_in, T=T, bug_compat=bug_compat)


def _sides(o, p, mask=None):
    """[(p . LHS(p), sum dc p^2 + c2 |Ldr p|^2)] for LHS_x and LHS_zd"""
    q2 = float((o.apply_op_Ldr(p) ** 2).sum())
    hth = np.zeros_like(p)
    if mask is None:
        hth[:, :o.t_in] = 1.0
    else:
        hth = mask.astype(np.float64)
    dcx = hth + (o.rho_u + o.rho_d) / 2
    x = (float((p * o.LHS_x(p, mask)).sum()), float((dcx * p * p).sum()) + o.rho / 2 * q2)
    zd = (float((p * o.LHS_zd(p)).sum()), o.rho_d / 2 * float((p * p).sum()) + o.mu_d2 * q2)
    return [("LHS_x", x), ("LHS_zd", zd)]


def _vectors(meta):
    rng = np.random.default_rng(7)
    shape = (3, int(meta["T"]), int(meta["n"]), 1)
    return [rng.standard_normal(shape), 100 + 50 * rng.random(shape)]


@pytest.mark.parametrize("bug_compat", [True, False])
@pytest.mark.parametrize("mode", ["knn", "line", "skip3"])
def test_pAp_equals_the_q_form_where_the_transpose_is_exact(g4_meta, mode, bug_compat):
    o = _oracle(g4_meta, mode, bug_compat)
    mask = np.repeat(g4_meta["mask"].astype(np.float64), 3, axis=0)
    for p in _vectors(g4_meta):
        for m in (None, mask):
            for name, (direct, folded) in _sides(o, p, m):
                assert abs(direct - folded) <= REL * abs(direct), (mode, bug_compat, name, direct, folded)


@pytest.mark.parametrize("bug_compat", [True, False])
def test_pAp_differs_from_the_q_form_under_transpose_by_gather(g4_meta, bug_compat):
    assert (g4_meta["knn_cl"] != -1).all() and g4_meta["knn_cl"].shape[1] == 5        # unpadded k = 4 table
    o = _oracle(g4_meta, "physical", bug_compat)
    assert o.WdT is o.Wd
    for p in _vectors(g4_meta):
        for name, (direct, folded) in _sides(o, p):
            assert abs(direct - folded) > 1e-6 * abs(direct), (bug_compat, name, direct, folded)


def test_query_id_of_the_barrier_count():
    """MGADMM_Q_LDS_CG_BARRIERS is item 17 in the header and in the ctypes binding."""
    import os
    import re
    from conftest import ROOT
    from mgadmm import _lib
    hdr = open(os.path.join(ROOT, "include", "mgadmm.h")).read()
    assert int(re.search(r"MGADMM_Q_LDS_CG_BARRIERS\s*=\s*(\d+)", hdr).group(1)) == 17 == _lib.Q_LDS_CG_BARRIERS
