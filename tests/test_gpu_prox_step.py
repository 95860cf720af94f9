"""The prox and dual steps on smooth, sparse-phi data (tests/prox_cases.py), where the soft threshold really thresholds.

a. the stand-alone prox (phi_direct, EpiPhiDirect of csrc/stream_kernels.h) at its exact edges: rho = 4, thr = 0.5, x = 0, so
   s = -gamma / 4 exactly, with s cycling through +-0, +-0.5, +-0.5 moved one float toward and away from 0, +-0.25, +-1, +-1e-30,
   +-denormals that are multiples of 4 ulp and +-(largest finite / 8) at every node and every t (t = 0 included).  Every
   operation is exact on these values (or rounds the same way in both formats: huge - 0.5 = huge), so the result equals the
   oracle's float64 phi_direct cast to the format bit for bit -- up to the sign of a zero: the reference's formula
   sign(s) u [u > 0] leaves -0.0 for a thresholded positive s, the kernels write +0.0 (no later step tells them apart), so
   both sides are compared after adding +0.0.  float32 and float64, B in {1, 3, 100, 200, 260} (the vector widths), with and
   without the cluster order, a kNN table and a line graph.
b. the one-step audit (prox_cases.audit_step) on every row of prox_cases.CASES: the state after 1 iteration (A1), one more
   iteration warm-started from it (B1), the same from the state after 5 (A5, B5); on windows 0, B // 2, B - 1 every entry of
   phi, gamma, gamma_u, gamma_d of B within its derived bound of the float64 recomputation from the solver's own numbers, no
   entry in the wrong class of the prox, at most 1 % of the entries left out of the class check.  LDS rows assert their instance
   and geometry as tests/test_gpu_lds_census.py does; the row with per-sample weights runs k_admm_lds_pp and audits every sample
   with its own threshold and rho.  Prints the largest error / bound of every quantity (DESIGN.md has the table).
c. 6 iterations of the same rows against the oracle (helpers.check_windows) at the tolerances of tests/test_gpu_lds_census.py
   (x 1e-5, zu 1e-4, phi 1e-3, lists rtol 1e-3; float64 rows: 1e-9, 1e-8, 1e-7, 1e-7), plus, for the functions of Ldr x (phi,
   the phi pair of the residual lists, DGTV, DGLR), the rounding of Ldr x itself: max(E_l) per entry (check_windows: ldr_allow).
"""
import numpy as np
import pytest
import torch

import lds_census as lc
import prox_cases as pc
from helpers import check_windows

pytestmark = pytest.mark.gpu

_DT = {"f32": (torch.float32, np.float32, np.uint32), "f64": (torch.float64, np.float64, np.uint64)}
LDS_SWITCHES = ("MGADMM_LDS_TPG", "MGADMM_LDS_NOSLOTS", "MGADMM_LDS_SB", "MGADMM_LDS_RAGGED", "MGADMM_LDS_TABLE_ORDER",
                "MGADMM_LDS_CHUNK", "MGADMM_LDS_BANK_SEARCH", "MGADMM_LDS_ASYNC")


@pytest.fixture
def env(monkeypatch):
    for k in LDS_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


# ------------------------------------------------------------------------------------------------- a. exact edges of the prox
def _edge_values(npdt):
    fi = np.finfo(npdt)
    half, sub = npdt(0.5), fi.smallest_subnormal
    pos = [npdt(0.0), half, np.nextafter(half, npdt(0)), np.nextafter(half, npdt(1)), npdt(0.25), npdt(1.0), npdt(1e-30),
           npdt(4) * sub, npdt(12) * sub, fi.tiny / npdt(2), fi.tiny - npdt(4) * sub, fi.max / npdt(8)]
    s = np.array(pos + [-v for v in pos], dtype=npdt)
    assert np.isfinite(s).all() and np.signbit(s[len(pos)]) and (s[7:11] > 0).all() and (s[7:11] < fi.tiny).all()
    return s


@pytest.mark.parametrize("graph", ["knn3", "line1"])
@pytest.mark.parametrize("reorder", [False, "cluster"])
@pytest.mark.parametrize("B", [1, 3, 100, 200, 260])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_phi_direct_exact_edges(dtype, B, reorder, graph):
    tdt, npdt, bits = _DT[dtype]
    N, T = 48, 12
    c = dict(kind=graph, N=N, T=T, t_in=6, abl="None", mu_d1=2, path="auto", dtype=dtype, reorder=reorder)
    w = pc.info(N, T, 2)
    assert w["rho"] == 4.0 and w["mu_d1"] / w["rho"] == 0.5
    blk = pc.product(c)
    o = pc.oracle_for(c, blk, w)
    s = _edge_values(npdt)
    V = len(s)
    b, t, n = np.meshgrid(np.arange(B), np.arange(T), np.arange(N), indexing="ij")
    x = torch.zeros((B, T, N, 1), dtype=tdt)
    seen = np.zeros((T, N, V), dtype=bool)
    for shift in range(0, V, B):                       # every (t, n) meets every value
        pick = (b + shift + n + 5 * t) % V
        seen[t, n, pick] = True
        gamma = (npdt(-4) * s[pick])[..., None]
        assert gamma.dtype == npdt and np.array_equal(gamma / npdt(4), -s[pick][..., None]) and np.isfinite(gamma).all()
        got = blk.phi_direct(x, torch.from_numpy(gamma)).numpy()
        want = o.phi_direct(np.zeros((B, T, N, 1)), gamma.astype(np.float64))
        assert np.array_equal(want, want.astype(npdt).astype(np.float64))      # the float64 result is a number of the format
        want = want.astype(npdt)
        assert got.dtype == npdt
        same = (got + npdt(0)).view(bits) == (want + npdt(0)).view(bits)
        if not same.all():
            i = tuple(np.argwhere(~same)[0])
            raise AssertionError((dtype, B, reorder, graph, f"{(~same).sum()} entries differ; first at (b, t, n, c) = {i}: "
                                  f"s = {float(s[pick][i[:3]])!r}, got {float(got[i])!r}, want {float(want[i])!r}"))
    assert seen.all()
    blk.close()


# -------------------------------------------------------------------------------------------------------- b., c. the solves
def _setup(c, env):
    from mgadmm import _lib
    for k, v in c["env"].items():
        env.setenv(k, v)
    tdt, npdt, _ = _DT[c["dtype"]]
    ref = pc.reference(c)
    y, mask = ref["y"], ref["mask"]
    yt = torch.from_numpy(y.astype(npdt))                               # in the compute dtype: the states keep their bits
    mt = None if mask is None else torch.from_numpy(mask.astype(npdt))
    blk = pc.product(c)
    h = blk._solver(1, tdt, c["B"])[0]
    if c["path"] == "lds":
        assert _lib.query(h, _lib.Q_LDS_INSTANCE) == -1 and _lib.lds_instance(h) is None, c["name"]          # no launch yet

    def solve(iters, warm=None):
        blk.max_ADMM_iter = iters
        blk.check_stop = False
        blk._reset_history()
        x = blk.solve(yt, mask=mt, per_sample_history=True, warm_start=warm, sample_params=c["sample_params"])[0]
        assert blk._solvers[(1, tdt)][0].value == h.value
        assert x.dtype == tdt and all(v.dtype == tdt for v in blk.state.values())
        return {k: v.clone() for k, v in blk.state.items()}

    def ran():
        """The kernels the row names really ran."""
        B = c["B"]
        if c["path"] == "stream":
            assert _lib.lib.mgadmm_solver_path(h, B) == _lib.PATH_STREAM, c["name"]
            return
        assert _lib.lib.mgadmm_solver_path(h, B) == _lib.PATH_LDS, c["name"]
        assert _lib.lds_instance(h) == c["expect"], (c["name"], _lib.lds_instance(h))
        assert _lib.query(h, _lib.Q_LDS_UNIT) == (2 if c["sample_params"] else 0), c["name"]
        nth, rows, ts, ghosts = lc.geometry(c)
        geo = [_lib.query(h, q) for q in (_lib.Q_LDS_THREADS, _lib.Q_LDS_ROWS, _lib.Q_LDS_ROW_STRIDE)]
        assert geo == [nth, rows, ts], (c["name"], "threads / rows / stride", geo, (nth, rows, ts), f"{ghosts} ghosts")

    return blk, ref, solve, ran


def _picked(state, idx):
    t = torch.as_tensor(idx)
    return {k: v[t].double().numpy() for k, v in state.items()}


@pytest.mark.parametrize("c", pc.CASES, ids=pc.case_id)
def test_one_step_audit(c, env):
    blk, ref, solve, ran = _setup(c, env)
    idx, eps = ref["idx"], pc.eps_of(c)
    w = pc.solver_weights(c, idx, eps)
    for k in pc.AUDIT_AT:
        A = solve(k)
        ran()
        Bs = solve(1, warm=A)
        ran()
        a = pc.audit_step(ref["o"], _picked(A, idx), _picked(Bs, idx), eps, w)
        print(f"\n[prox audit] {c['name']} iteration {k}: err/bound " + " ".join(f"{q} {v:.3f}" for q, v in a["ratio"].items())
              + f"; classes {'/'.join(f'{v:.2f}' for v in a['shares'])}; left out {a['left_out']:.4f}; mismatches {a['mismatch']}")
        assert not any(a["bad"].values()), (c["name"], k, "entries over their bound", a["bad"], a["ratio"])
        assert a["mismatch"] == 0, (c["name"], k, "entries in the wrong class of the prox", a["mismatch"])
        assert a["left_out"] <= pc.MAX_NEAR, (c["name"], k, a["left_out"])
        assert a["shares"][0] >= pc.MIN_SHARE, (c["name"], k, a["shares"])         # (the solver's own s thresholds as well)
    blk.close()


@pytest.mark.parametrize("c", pc.CASES, ids=pc.case_id)
def test_trajectory_on_smooth_data(c, env):
    blk, ref, solve, ran = _setup(c, env)
    idx, eps, f32 = ref["idx"], pc.eps_of(c), c["dtype"] == "f32"
    state = solve(pc.ITERS)
    ran()
    x = state["x"]
    wr = pc.solver_weights(c, idx, eps)
    El = max(pc.audit_step(ref["o"], ref["states"][k], ref["states"][k + 1], eps, wr)["E_l_max"] for k in pc.AUDIT_AT)
    zu_tol, phi_tol = (1e-4, 1e-3) if f32 else (1e-8, 1e-7)
    for p, o, xo in ref["groups"]:
        sel = [idx[j] for j in p]
        tag = f"{c['name']} windows {sel}"
        got = _picked(state, sel)
        rel = {k: float(np.linalg.norm(got[k] - o.state[k]) / np.linalg.norm(o.state[k])) for k in o.state}
        allow = np.sqrt(o.state["phi"].size) * El / np.linalg.norm(o.state["phi"])
        print(f"\n[prox trajectory] {tag}: " + " ".join(f"{k} {v:.2e}" for k, v in rel.items()) + f"; max E_l {El:.2e}, phi allowance {allow:.2e}")
        if f32:
            # (finite-termination counts: as in test_gpu_lds_census.py on the LDS rows, test_gpu_stream_census.py on the skip-1 line graph)
            check_windows(tag, blk, x, sel, o, xo, abl=c["abl"], finite_termination_rule=c["path"] == "lds" or c["kind"] == "line1",
                          ldr_allow=El)
        else:
            check_windows(tag, blk, x, sel, o, xo, xtol=1e-9, htol=1e-7, slack=0, abl=c["abl"], ldr_allow=El)
        assert rel["zu"] <= zu_tol, (tag, "zu", rel["zu"])
        assert rel["phi"] <= phi_tol + allow, (tag, "phi", rel["phi"], allow)
    blk.close()
