"""Smooth, sparse-phi problems for the prox and dual steps, and a one-step audit of those steps in float64.

Every other solve-level test feeds the solver rough data (100 + 50 rand): there |Ldr x| is about 50 against a prox threshold
mu_d1 / rho of about 0.5, the soft threshold only shifts its argument and its zero branch hardly fires.  The inputs here are
smooth in time at the same level (about 100), so Ldr x = x_t - sum w x_{t-1} cancels down to a few tenths, most of it lies
below the threshold and phi is sparse: the regime the DGTV term exists for, and the one where float32 loses digits.

  smooth_inputs   the data
  CASES           the problems: rows of tests/lds_census.py (LDS path) and small graphs of its builders (streaming path,
                  float32 / float32 cluster order / float64), one row with per-sample weights
  audit_step      given the state a solver exported before (A) and after (B) ONE iteration, recompute every element-wise step
                  of that iteration (oracle/admm_oracle.py, combined_loop: phi, gamma, gamma_u, gamma_d) in float64 from the
                  solver's own numbers, with a derived error bound per entry, and check the branch the prox took
  step_in_float32 the same step in correctly rounded float32 (and four wrong variants of it): what the audit must accept (and refuse)
  reference       the float64 oracle on a case's audited windows: trajectory, states after 1, 2, 5, 6 iterations

Plain numpy; tests/test_prox_cases_cpu.py checks the cases and the audit itself, tests/test_gpu_prox_step.py runs them on the GPU.

The bounds (eps = 2^-23 or 2^-52, the spacing of the format at 1; one rounding is eps / 2 relative):
  l = Ldr x_B        E_l = (d + 3) eps (|Ldr| |x_B|): d the longest row of Ldr; a sum of d products in any order, with or without
                     fused multiply-add, errs by at most d eps / 2 (1 + O(eps)) of the sum of absolute terms; the rest is slack
                     that also pays for the two roundings of |l| in s and u below
  phi                E_phi = E_l + 2 eps (|gamma_A| / rho + thr): the soft threshold is 1-Lipschitz in s and in thr; the quotient,
                     s, u and thr are one rounding each
  gamma              E_gamma = rho E_l + 4 eps (|gamma_A| + rho |phi_B - l|): difference, product, sum
  gamma_u, gamma_d   4 eps (|gamma_A| + rho (|x_B| + |z_B|))
rho and mu_d1 are the numbers the solver holds: the weights rounded to its format (solver_weights).
"""
import math

import numpy as np

import lds_census as lc

F32_EPS, F64_EPS = 2.0 ** -23, 2.0 ** -52
ITERS = 6                   # trajectory length
AUDIT_AT = (1, 5)           # iteration indices audited: from the state after 1 (5) iterations to the one after 2 (6)
STATE_ITERS = (1, 2, 5, 6)
MIN_SHARE, MAX_NEAR = 0.05, 0.01


# ---------------------------------------------------------------------------------------------------------------- inputs
def smooth_inputs(B, T, N, t_in, task, seed=0, noise=0.4):
    """(y, mask) in float64: x_true[b, t, n] = L_b + s_b t + noise e, L_b ~ U(100, 120), s_b ~ 0.3 N(0, 1), e ~ N(0, 1).
    'pred': y = x_true[:, :t_in], mask None; 'mask': y = x_true mask with 40 % of the entries dropped."""
    rng = np.random.default_rng(seed)
    L = rng.uniform(100.0, 120.0, (B, 1, 1, 1))
    s = 0.3 * rng.standard_normal((B, 1, 1, 1))
    e = rng.standard_normal((B, T, N, 1))
    x_true = L + s * np.arange(T, dtype=np.float64).reshape(1, T, 1, 1) + noise * e
    if task == "pred":
        return x_true[:, :t_in].copy(), None
    mask = (rng.random((B, T, N, 1)) >= 0.4).astype(np.float64)
    return x_true * mask, mask


def info(N, T, mu_d1):
    """The weights of tests/test_gpu_lds_census.py (_info) with the case's mu_d1."""
    r = math.sqrt(N / T)
    return dict(rho=2 * r, rho_u=3 * r, rho_d=2 * r, mu_u=1, mu_d1=mu_d1, mu_d2=1)


# ----------------------------------------------------------------------------------------------------------------- cases
def _case(name, kind, N, T, t_in, abl, task, B, mu_d1, path, dtype="f32", reorder=None, indeg=None, env=None, expect=None,
          sample_params=None, noise=0.4):
    return dict(name=name, kind=kind, N=N, T=T, t_in=t_in, abl=abl, task=task, B=B, mu_d1=mu_d1, path=path, dtype=dtype,
                reorder=reorder, indeg=indeg, env=env or {}, expect=expect, sample_params=sample_params, noise=noise)


def _lds(name, expect, mu_d1, **kw):
    """A row of lc.CENSUS (found by its instance) as it stands: N, T, t_in, graph, ablation, task, B, env."""
    r, = [r for r in lc.CENSUS if r["expect"] == expect]
    assert r["abl"] in ("None", "DGLR"), (expect, "no phi")
    return _case(name, r["kind"], r["N"], r["T"], r["t_in"], r["abl"], r["task"], r["B"], mu_d1, "lds", indeg=r["indeg"],
                 env=r["env"], expect=expect, **kw)


def _small(kind, N, abl, task, mu, indeg=None):
    rows = []
    for tag, dtype, reorder in (("f32", "f32", None), ("f32-cluster", "f32", "cluster"), ("f64", "f64", None)):
        rows.append(_case(f"stream-{tag}-{kind}-N{N}", kind, N, 24, 12, abl, task, 3, mu, "stream", dtype, reorder, indeg))
    return rows


def _r(N, T):
    return math.sqrt(N / T)


# mu_d1: 6 on kNN, uniform and physical graphs, 2 on line graphs, where the oracle alone then meets the conditions of
# tests/test_prox_cases_cpu.py (every class of the prox populated).  The threshold mu_d1 / rho = mu_d1 / (2 sqrt(N / T)) grows as
# N / T falls while the noise stays at 0.4, so with mu_d1 = 6 the small graphs (N <= 96: thr 1.5 ... 2.7), the knnpad row (N 60:
# thr 1.9) and the N 180, T 36 rows (thr 1.3) put 95 ... 100 % of the entries in the zero class at both audited iterations;
# those rows carry the mu_d1 that brings thr back to about 0.6 (marked "thr"), and so does the N 30 line graph.
CASES = [
    _lds("lds-uni8-slots", lc.uni(8, 1024, True, 0), 6),                        # N 341, T 24
    _lds("lds-uni8-noslots", lc.uni(8, 1024, False, 3), 6),                     # N 500, T 16
    _lds("lds-uni12-640", lc.uni(12, 640, True, 0), 3),                         # N 180, T 36; thr 0.67
    _lds("lds-uni12-1024-N512", lc.uni(12, 1024, False, -1), 6),                # N 512, T 24, 0 ghosts, B 5
    _lds("lds-knnpad-mask", lc.inst(2, False, 1024, False), 2),                 # N 60, ragged rows with pads; thr 0.63
    _lds("lds-physical-dglr", lc.inst(3, False, 1024, False), 6),               # N 100
    _lds("lds-line1", lc.inst(6, True, 1024, False), 2),                        # N 200
    _lds("lds-line3-dglr", lc.inst(8, True, 1024, False), 2),                   # N 300
    _lds("lds-sb-uni12-640", lc.inst(12, False, 640, True), 3),                 # N 180, T 36, MGADMM_LDS_SB; thr 0.67
    # per-sample weights (k_admm_lds_pp): every sample its own threshold mu_d1 / rho = 1 / r, 3 / r, 3 / r and its own rho
    _lds("lds-pp-knn3", lc.inst(4, False, 1024, False), 6,
         sample_params=dict(mu_d1=[1.0, 6.0, 12.0], rho=[_r(150, 24), 2 * _r(150, 24), 4 * _r(150, 24)])),
]
CASES += _small("uniform", 43, "None", "mask", 1.5, indeg=6)      # thr 0.56
CASES += _small("uniform", 96, "None", "pred", 2.5, indeg=5)      # thr 0.63
CASES += _small("knn3", 30, "None", "pred", 1.5)                  # thr 0.67
CASES += _small("knnpad", 60, "None", "mask", 2)                  # thr 0.63
CASES += _small("line1", 30, "None", "pred", 1.2)                 # thr 0.54 (mu_d1 2: thr 0.89, 3 % in the positive class)
CASES += _small("line3", 60, "DGLR", "pred", 2)
assert len({c["name"] for c in CASES}) == len(CASES)


def case_id(c):
    return c["name"]


def windows(c):
    """The audited windows: 0, B // 2, B - 1."""
    return sorted({0, c["B"] // 2, c["B"] - 1})


def eps_of(c):
    return F32_EPS if c["dtype"] == "f32" else F64_EPS


def case_inputs(c):
    return smooth_inputs(c["B"], c["T"], c["N"], c["t_in"], c["task"], seed=0, noise=c["noise"])


def sample_info(c, b):
    """The ADMM weights of sample b."""
    w = info(c["N"], c["T"], c["mu_d1"])
    for k, v in (c["sample_params"] or {}).items():
        w[k] = float(v[b])
    return w


def solver_weights(c, idx, eps):
    """{name: (len(idx), 1, 1, 1) float64}: the weights of the samples `idx` as a solver of that format holds them."""
    cast = np.float32 if eps == F32_EPS else np.float64
    ws = [sample_info(c, b) for b in idx]
    return {k: np.array([cast(w[k]) for w in ws], dtype=np.float64).reshape(-1, 1, 1, 1) for k in ws[0]}


def product(c, **kw):
    """mgadmm.ADMM_algorithm of the case (constructing it needs no GPU)."""
    import mgadmm
    import torch
    N, T, kind = c["N"], c["T"], c["kind"]
    common = dict(ablation=c["abl"], t_in=c["t_in"], T=T, record_cg_coeffs=False, path=c["path"],
                  compute_dtype=torch.float32 if c["dtype"] == "f32" else torch.float64)
    if c["reorder"] is not None:
        common["reorder"] = c["reorder"]
    common.update(kw)
    w = info(N, T, c["mu_d1"])
    if kind == "physical":
        ue, ud = lc.physical_graph(N)
        return mgadmm.ADMM_algorithm({"n_nodes": N, "u_edges": ue, "u_dist": ud}, w, use_kNN=False, **common)
    cl, dl = lc.tables_for(c)
    return mgadmm.ADMM_algorithm({"n_nodes": N}, w, use_kNN=True, k=cl.shape[1] - 1, tables=(cl, dl),
                                 use_line_graph=kind.startswith("line"), skip_connection=3 if kind == "line3" else 1, **common)


def oracle_for(c, blk, w):
    """The float64 oracle on the tables of `blk` with the weights `w`."""
    from oracle import admm_oracle as orc
    cl = blk.connect_list.numpy()
    kw = dict(ablation=c["abl"], t_in=c["t_in"], T=c["T"])
    if c["kind"].startswith("line"):
        return orc.OracleADMM(cl, blk.u_ew[0].numpy(), None, w, mode="line", skip_connection=blk.skip_connection, **kw)
    mode = "physical" if c["kind"] == "physical" else "knn"
    return orc.OracleADMM(cl, blk.u_ew[0].numpy(), blk.d_ew[0].numpy(), w, mode=mode, **kw)


# ------------------------------------------------------------------------------------------------------------- reference
_REF = {}


def reference(c):
    """The oracle on the audited windows of case c, computed once per problem (cases that differ only in path, format and node
    order share it) and left unchanged: dict(idx, y, mask, groups=[(positions in idx, oracle after ITERS iterations, x)],
    states={n: state after n iterations, (len(idx), T, N, 1)}, o=an oracle for its operators)."""
    sp = c["sample_params"]
    key = (c["kind"], c["N"], c["T"], c["t_in"], c["abl"], c["task"], c["B"], c["indeg"], c["mu_d1"], c["noise"],
           None if sp is None else tuple((k, tuple(v)) for k, v in sorted(sp.items())))
    if key in _REF:
        return _REF[key]
    idx = windows(c)
    y, mask = case_inputs(c)
    blk = product(c)
    pos = [[j] for j in range(len(idx))] if sp else [list(range(len(idx)))]
    groups, states = [], {n: {} for n in STATE_ITERS}
    for p in pos:
        w = sample_info(c, idx[p[0]])
        sel = [idx[j] for j in p]
        yy, mm = y[sel], None if mask is None else mask[sel]
        for n in STATE_ITERS:
            o = oracle_for(c, blk, w)
            x = o.combined_loop(yy, mask=mm, n_iters=n)
            for k, v in o.state.items():
                states[n].setdefault(k, []).append(v)
        groups.append((p, o, x))                                        # (the last run: ITERS iterations)
    assert STATE_ITERS[-1] == ITERS
    states = {n: {k: np.concatenate(v) for k, v in st.items()} for n, st in states.items()}
    ref = dict(idx=idx, y=y, mask=mask, groups=groups, states=states, o=groups[0][1])
    _REF[key] = ref
    return ref


# ----------------------------------------------------------------------------------------------------------------- audit
def soft(s, thr):
    return np.sign(s) * np.maximum(np.abs(s) - thr, 0.0)


def abs_ldr(o, ax):
    """(|Ldr| ax, d): the operator with absolute weights on ax >= 0, and the longest row of Ldr."""
    out = np.zeros_like(ax)
    if o.mode == "line":
        for t in range(1, ax.shape[1]):
            out[:, t] = ax[:, t]
            for s in range(min(t, o.skip)):
                out[:, t] += abs(float(o.wt[t, s])) * ax[:, t - 1 - s]
        return out, 1 + o.skip
    Wa = abs(o.Wd)
    out[:, 1:] = ax[:, 1:] + o._sp(Wa, ax[:, :-1])
    return out, 1 + int(np.diff(o.Wd.indptr).max())


def audit_step(o, A, B, eps, w):
    """One ADMM iteration from state A to state B (dicts of float64 arrays (n, T, N, 1) holding the solver's numbers exactly),
    audited in float64.  `o`: an OracleADMM, used for Ldr and the ablation only; `w`: the solver's weights per sample
    (solver_weights).  Returns dict(err, bound: {quantity: per-entry arrays}, ratio: {quantity: largest err / bound},
    bad: entries over their bound, mismatch: entries outside E_phi of +-thr whose phi_B is in the wrong class (not exactly 0.0
    in the zero class, not of the sign of s otherwise), left_out: share of entries within E_phi of +-thr, shares: (zero,
    positive, negative) share of the entries t >= 1 by the class of s)."""
    has_phi, has_zd = o.ablation in ("None", "DGLR"), o.ablation != "DGLR"
    f = lambda a: np.asarray(a, dtype=np.float64)
    xB = f(B["x"])
    err, bound = {}, {}
    out = dict(err=err, bound=bound, mismatch=0, left_out=0.0, shares=None)
    E_l = 0.0
    if has_phi:
        rho, thr = w["rho"], w["mu_d1"] / w["rho"]
        l = o.apply_op_Ldr(xB)
        al, d = abs_ldr(o, np.abs(xB))
        E_l = (d + 3) * eps * al
        gA, phiB = f(A["gamma"]), f(B["phi"])
        s = l - gA / rho
        E_phi = E_l + 2 * eps * (np.abs(gA) / rho + thr)
        err["phi"], bound["phi"] = np.abs(phiB - soft(s, thr)), E_phi
        err["gamma"] = np.abs(f(B["gamma"]) - (gA + rho * (phiB - l)))
        bound["gamma"] = rho * E_l + 4 * eps * (np.abs(gA) + rho * np.abs(phiB - l))
        clear = np.abs(np.abs(s) - thr) > E_phi
        zero = np.abs(s) < thr
        wrong = np.where(zero, phiB != 0.0, np.sign(phiB) != np.sign(s))
        out["mismatch"] = int((clear & wrong).sum())
        out["left_out"] = float(1.0 - clear.mean())
        s1, z1 = s[:, 1:], zero[:, 1:]
        out["shares"] = (float(z1.mean()), float((~z1 & (s1 > 0)).mean()), float((~z1 & (s1 < 0)).mean()))
    for g, z, r in (("gamma_u", "zu", "rho_u"),) + ((("gamma_d", "zd", "rho_d"),) if has_zd else ()):
        gA, zB = f(A[g]), f(B[z])
        err[g] = np.abs(f(B[g]) - (gA + w[r] * (xB - zB)))
        bound[g] = 4 * eps * (np.abs(gA) + w[r] * (np.abs(xB) + np.abs(zB)))
    out["E_l_max"] = float(np.max(E_l))
    out["bad"] = {k: int((err[k] > bound[k]).sum()) for k in err}
    with np.errstate(divide="ignore", invalid="ignore"):
        out["ratio"] = {k: float(np.max(np.where(err[k] > 0, err[k] / bound[k], 0.0))) for k in err}
    return out


def audit_ok(a, max_left_out=MAX_NEAR):
    return not any(a["bad"].values()) and a["mismatch"] == 0 and a["left_out"] <= max_left_out


VARIANTS = ("zero class returns s", "sign dropped", "threshold mu_d1 / rho_u", "gamma from phi_A")


def step_in_float32(o, A, nxt, w, variant=None):
    """State B of a float32 solver: x, zu, zd of `nxt` and gamma_u, gamma_d, phi, gamma computed from them and from A (all rounded
    to float32 first) in float32, every operation rounded once.  `variant`: one of VARIANTS, a wrong prox or dual step."""
    assert variant is None or variant in VARIANTS
    has_phi, has_zd = o.ablation in ("None", "DGLR"), o.ablation != "DGLR"
    f = lambda a: np.asarray(a, dtype=np.float32)
    wf = {k: f(v) for k, v in w.items()}
    B = {k: f(nxt[k]) for k in ("x", "zu", "zd")}
    B["gamma_u"] = f(A["gamma_u"]) + wf["rho_u"] * (B["x"] - B["zu"])
    B["gamma_d"] = f(A["gamma_d"]) + wf["rho_d"] * (B["x"] - B["zd"]) if has_zd else f(A["gamma_d"])
    if has_phi:
        l = o.apply_op_Ldr(B["x"])
        assert l.dtype == np.float32
        gA = f(A["gamma"])
        thr = wf["mu_d1"] / (wf["rho_u"] if variant == VARIANTS[2] else wf["rho"])
        s = l - gA / wf["rho"]
        u = np.abs(s) - thr
        sgn = np.float32(1) if variant == VARIANTS[1] else np.where(s > 0, np.float32(1), np.float32(-1))
        phi = np.where(u > 0, sgn * u, s if variant == VARIANTS[0] else np.float32(0)).astype(np.float32)
        B["phi"] = phi
        B["gamma"] = gA + wf["rho"] * ((f(A["phi"]) if variant == VARIANTS[3] else phi) - l)
    assert all(v.dtype == np.float32 for v in B.values())
    return {k: v.astype(np.float64) for k, v in B.items()}
