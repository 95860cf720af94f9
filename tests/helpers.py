"""Shared builders for the parity tests: the same problem as an oracle instance (CPU restatement,
test infrastructure) and as a product instance (HIP path through the C ABI)."""
import numpy as np
import torch

from conftest import admm_info_from
from oracle import admm_oracle as orc


def rel(a, b):
    a = np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu().numpy() if torch.is_tensor(b) else b, dtype=np.float64)
    n = np.linalg.norm(b)
    d = np.linalg.norm(a - b)
    return d / n if n > 0 else d


def _tiny(**kw):
    """The two-node instance of the CPU checks of solve()'s arguments."""
    from mgadmm.ADMM import ADMM_algorithm
    cl = torch.tensor([[0, 1], [1, 0]])
    return ADMM_algorithm({"n_nodes": 2}, dict(rho=1, rho_u=1, rho_d=1, mu_u=1, mu_d1=1, mu_d2=1), use_kNN=True,
                          u_sigma=1.0, d_sigma=1.0, tables=(cl, torch.tensor([[0.0, 1.0], [0.0, 1.0]])), **kw)


def make_oracle(meta, mode, ablation="None", bug_compat=True, prefix="knn", T=None, t_in=None):
    info = admm_info_from(meta)
    T = int(meta["T"]) if T is None else T
    t_in = int(meta["t_in"]) if t_in is None else t_in
    if mode == "knn":
        return orc.OracleADMM(meta["knn_cl"], meta["knn_u_ew"], meta["knn_d_ew"], info, mode="knn", ablation=ablation,
                              t_in=t_in, T=T, bug_compat=bug_compat)
    if mode == "physical":
        return orc.OracleADMM(meta["phys_cl"], meta["phys_u_ew"], meta["phys_d_ew"], info, mode="physical",
                              ablation=ablation, t_in=t_in, T=T, bug_compat=bug_compat)
    return orc.OracleADMM(meta["knn_cl"], meta["knn_u_ew"], None, info, mode="line", ablation=ablation, t_in=t_in, T=T,
                          skip_connection=1 if mode == "line" else 3)


def make_product(meta, mode, ablation="None", compute_dtype=torch.float32, bug_compat=True, T=None, t_in=None, **kw):
    """mgadmm.ADMM_algorithm on the golden tables (tables injected so both sides see identical weights)."""
    from mgadmm.ADMM import ADMM_algorithm
    info = admm_info_from(meta)
    T = int(meta["T"]) if T is None else T
    t_in = int(meta["t_in"]) if t_in is None else t_in
    n = int(meta["n"])
    gi = {"n_nodes": n}
    if mode == "physical":
        cl, dl = torch.from_numpy(meta["phys_cl"]), torch.zeros(meta["phys_cl"].shape)
        u_ew, d_ew = meta["phys_u_ew"], meta["phys_d_ew"]
    else:
        cl, dl = torch.from_numpy(meta["knn_cl"]), torch.zeros(meta["knn_cl"].shape)
        u_ew, d_ew = meta["knn_u_ew"], meta.get("knn_d_ew") if hasattr(meta, "get") else meta["knn_d_ew"]
    blk = ADMM_algorithm(gi, info, use_kNN=(mode != "physical"), k=cl.shape[1] - 1, u_sigma=1.0, d_sigma=1.0,
                         ablation=ablation, t_in=t_in, T=T, use_line_graph=mode in ("line", "skip3"),
                         skip_connection=3 if mode == "skip3" else 1, tables=(cl, dl + 1.0),
                         compute_dtype=compute_dtype, bug_compat=bug_compat, **kw)
    # overwrite the weight tables with the golden ones (float32, exactly what the reference used)
    blk.u_ew = torch.from_numpy(np.asarray(u_ew, dtype=np.float32)).unsqueeze(0).repeat(T, 1, 1)
    if mode in ("knn", "physical"):
        blk.d_ew = torch.from_numpy(np.asarray(d_ew, dtype=np.float32)).unsqueeze(0).repeat(T - 1, 1, 1)
    return blk


def meta_from_g2(g):
    """g2/g3 fixture -> dict with the keys make_oracle/make_product expect."""
    d = {k: g[k] for k in ("rho", "rho_u", "rho_d", "mu_u", "mu_d1", "mu_d2", "T", "t_in", "n")}
    d["knn_cl"] = d["phys_cl"] = g["cl"]
    d["knn_u_ew"] = d["phys_u_ew"] = g["u_ew"]
    if g["d_ew"].ndim == 2:
        d["knn_d_ew"] = d["phys_d_ew"] = g["d_ew"]
    else:
        d["knn_d_ew"] = d["phys_d_ew"] = None
    return d


def case_inputs(meta, task, np_dtype):
    t_in = int(meta["t_in"])
    if task == "pred":
        return meta["x_true"][:, :t_in].astype(np_dtype), None
    mask = meta["mask"]
    return (meta["x_true"] * mask).astype(np_dtype), mask


F32_EPS = 2.0 ** -23


def finite_termination(h, nm, n_it):
    """(iters, windows) bool: the oracle's CG solve ended with a step that cut ||r|| by more than float32 resolves
    (||r_k|| / ||r_k-1|| = sqrt(beta_k) < 2^-23) -- exact termination on a system with few distinct eigenvalues, not
    convergence.  The float32 residual of that step is rounding only."""
    w = nm.replace("CG_iter", "beta")
    its = np.array(getattr(h, nm)).reshape(n_it, -1)
    out = np.zeros(its.shape, dtype=bool)
    for i, be in enumerate(getattr(h, w)):
        for j in range(its.shape[1]):
            k = its[i, j]
            out[i, j] = k > 0 and np.sqrt(be[k - 1, j]) < F32_EPS
    return out


def check_windows(tag, blk, x, idx, o, xo, xtol=1e-5, htol=1e-3, slack=1, abl="None", finite_termination_rule=False, ldr_allow=0.0):
    """GPU batch result `x` (+ blk.metrics_per_sample, blk.CG_iter_*) against the oracle run on windows `idx`.
    Tolerances of the BASELINE configs (float32 kernels vs the float64 oracle): x per sample, every history list, CG counts
    (the diagonal x solve of 'DGTV' / 'UT' gets the +-2 of check_solve in test_gpu_parity.py).
    finite_termination_rule: a solve whose float64 count is a finite-termination count (finite_termination) may also lie
    in [ref - 1, 2 ref + 1], the bound test_gpu_random.py sets for such counts: float32 loses the exact termination and
    runs on until its recursive residual passes the tolerance.
    ldr_allow: E, the largest rounding error of an entry of Ldr x in the solver's format (tests/prox_cases.py: E_l).  On smooth
    data Ldr x is small against ||x||, and the quantities that are functions of it get E on top of their tolerance: a norm over
    M entries (the phi pair of the residual lists) sqrt(M) E, the sum of |Ldr x| (DGTV) E per entry, and the sum of squares
    (DGLR), a squared norm n^2, d (2 n + d) with d = sqrt(M) E.  0 (the default) changes nothing."""
    from mgadmm import _lib as L
    has_phi, has_zd = abl in ("None", "DGLR"), abl != "DGLR"
    idx = np.asarray(idx)
    xg = x[torch.as_tensor(idx, device=x.device)].double().cpu().numpy()
    err = np.linalg.norm((xg - xo).reshape(len(idx), -1), axis=1) / np.linalg.norm(xo.reshape(len(idx), -1), axis=1)
    assert err.max() < xtol, (tag, "x", err.max())
    mps = blk.metrics_per_sample[:, :, idx]                  # (iters, NMETRIC, k) per-sample sums
    h = o.hist
    n_it = len(h.p_res_list)
    assert mps.shape[0] == n_it
    # norms of DIFFERENCES of float32 vectors (||x - x_old||, ||z - z_old||, ...) carry the rounding of the vectors
    # themselves: 2 ulp of float32 relative to ||x_ref|| is the resolution (cfg4, iteration 0: ||x1 - x0|| = 1.4 on
    # ||x|| = 5.4e5 -- the initial guess almost solves the first x-update -- measured difference 0.03 = 6e-8 ||x||)
    floor = 1e-7 * float(np.linalg.norm(xo))
    norm = lambda m: np.sqrt(mps[:, m].sum(1))
    mean = lambda m: mps[:, m].mean(1)
    res = [(L.M_PRI_ZU, L.M_DUAL_ZU)] + [(L.M_PRI_PHI, L.M_DUAL_PHI)] * has_phi + [(L.M_PRI_ZD, L.M_DUAL_ZD)] * has_zd
    pri = np.stack([norm(p) for p, _ in res], 1)
    dual = np.stack([norm(d) for _, d in res], 1)
    per_window = xo[0].size                                   # entries of one window
    at = np.full(len(res), floor)
    if has_phi:
        at[1] += np.sqrt(per_window * len(idx)) * ldr_allow
    for j in range(len(res)):
        np.testing.assert_allclose(pri[:, j], np.array(h.p_res_list)[:, j], rtol=htol, atol=at[j], err_msg=f"{tag} primal residuals, column {j}")
        np.testing.assert_allclose(dual[:, j], np.array(h.d_res_list)[:, j], rtol=htol, atol=at[j], err_msg=f"{tag} dual residuals, column {j}")
    np.testing.assert_allclose(norm(L.M_XSHIFT), np.array(h.x_shift_list), rtol=htol, atol=floor, err_msg=f"{tag} x shift")
    np.testing.assert_allclose(norm(L.M_RECOVER), np.array(h.recover_list), rtol=htol, atol=floor, err_msg=f"{tag} ||Hx-y||")
    np.testing.assert_allclose(mean(L.M_GLR), np.array(h.GLR_list), rtol=htol, err_msg=f"{tag} GLR")
    if has_phi:
        np.testing.assert_allclose(mean(L.M_DGTV), np.array(h.DGTV_list), rtol=htol, atol=per_window * ldr_allow, err_msg=f"{tag} DGTV")
    if has_zd:
        d = np.sqrt(per_window) * ldr_allow
        for i, (g, r) in enumerate(zip(mean(L.M_DGLR), h.DGLR_list)):
            np.testing.assert_allclose(g, r, rtol=htol, atol=d * (2 * np.sqrt(r) + d), err_msg=f"{tag} DGLR, iteration {i}")
    for nm in ("CG_iter_x", "CG_iter_zu") + ("CG_iter_zd",) * has_zd:
        got = torch.stack(getattr(blk, nm)).numpy()[:, idx]
        ref = np.array(getattr(h, nm)).reshape(n_it, -1)
        s = slack if nm != "CG_iter_x" or has_phi else max(slack, 2)
        assert (got > 0).all(), (tag, nm, "CG did not converge")
        ok = np.abs(got - ref) <= s
        if finite_termination_rule and s == slack:         # (the diagonal x solves keep their own slack)
            ok |= finite_termination(h, nm, n_it) & (got >= ref - 1) & (got <= 2 * ref + 1)
        assert ok.all(), (tag, nm, np.abs(got - ref).max())
