"""Problems of the adaptive-penalty tests (tests/test_gpu_adaptive_rho.py, tests/test_lds_adapt_cpu.py): the fixture of
param_schedule_cases.py (tables of g4_meta.npz, N = 30, T = 24; the 8 inputs of g5_batched.npz; four cases), the rule of
csrc/lds_adapt.h restated in numpy, and the float64 twin: the oracle whose three penalties are properties that replay the
rule over hist.p_res_list / d_res_list.  Plain builders, no device needed.

The comparisons against the twin clamp the penalties (rho_min / rho_max, TWIN_CLAMPS, as factors of the fixture's values).
rho_u / 2 and rho_d / 2 are the diagonal shifts of the zu and zd CG systems and part of the x system's: far below the
fixture's values those systems are badly conditioned, their solves take 2 ... 3 x the iterations, and a float32 CG recursion
then passes CG_tol a few iterations from the float64 one, whatever kernel runs it -- the +-1 on CG counts of the project's
comparisons holds where the project's other twins stand, which vary the weights by factors 0.5 ... 2 (the rhos) and
0.25 ... 4 (all six) of these very values (ROWS of test_gpu_sample_params.py).  So: with a phi pair ('None', 'DGLR') rho_u and
rho_d stay within [0.5, 2] and rho, which enters the x system as the factor of Ldr^T Ldr and the threshold only, within
[1/16, 16]; without one ('DGTV': only rho_u and rho_d adapt, and within [0.5, 2] they only fall) all stay within [0.25, 4].
The clamps are part of the feature and are reached in every case.

The triple (every, mu, tau) of a case is the first of CANDIDATES for which, over all 8 samples of the case and K = 20
iterations, every decision of the twin lies at least MARGIN = 1 % (in the residual norms) from both of its thresholds --
float32 residuals agree with the oracle's to 1e-3, so the float32 solve takes the same decisions -- and steps in both
directions occur; `triple(i)` raises when none does.  Searched on the CPU over every in (4, 5), mu in (1.25, 1.5, 2), tau in
(2, 4) -- (smallest margin, steps up, steps down) of the 8 samples under the clamps:
    (4, 1.25, 2)   knn-None 3.3 %, 13, 41    knn-DGLR 1.1 %, 8, 38    line-None 1.8 %, 12, 40    physical-DGTV: no step upwards
    (4, 1.5, 4)    physical-DGTV 5.1 %, 6, 22
so the three cases with phi take (4, 1.25, 2) and physical-DGTV takes (4, 1.5, 4); the twins' largest CG count is 46 of 100.
(4, 10, 2), the textbook values, takes no step upwards on this fixture within 20 iterations.  Without clamps the penalties
fall to 1/16 of the fixture's values before any comes back up; that run is what the chain tests use (they need no twin).
tau = 2 and 4 are powers of two: a penalty is its start value times a power of two, or a clamp."""
import functools

import numpy as np

import param_schedule_cases as pc
from helpers import make_oracle

NAMES, CASES, IDS, K = pc.NAMES, pc.CASES, pc.IDS, pc.K
meta, inputs, info = pc.meta, pc.inputs, pc.info
F32_X_TOL, F32_HIST_RTOL = pc.F32_X_TOL, pc.F32_HIST_RTOL
CANDIDATES = [(4, 1.25, 2.0), (4, 1.5, 4.0), (4, 2.0, 2.0), (4, 1.25, 4.0)]
# factors (lo, hi) of the fixture's rho, rho_u, rho_d the twin comparisons clamp to (module docstring), by "has a phi pair"
TWIN_CLAMPS = {True: ((1 / 16, 16.0), (0.5, 2.0), (0.5, 2.0)), False: ((0.25, 4.0), (0.25, 4.0), (0.25, 4.0))}
MARGIN = 0.01
RHO_MIN, RHO_MAX = 1e-6, 1e6
PAIRS = (("rho_u", 1, 2), ("rho", 3, 4), ("rho_d", 5, 6))      # penalty, MGADMM_M_PRI_*, MGADMM_M_DUAL_* of its pair


def has(abl):
    return abl in ("None", "DGLR"), abl != "DGLR"


# ------------------------------------------------------------------------------------------------ the rule in numpy
def balance(r, pri2, dual2, mu, tau, lo=RHO_MIN, hi=RHO_MAX):
    """One pair, elementwise on float64 arrays: the multiplications and comparisons of ldsadapt::balance in their order."""
    r, pri2, dual2 = (np.asarray(v, dtype=np.float64) for v in (r, pri2, dual2))
    mu, tau = np.float64(mu), np.float64(tau)
    tau_inv = np.float64(1.0) / tau
    with np.errstate(invalid="ignore", over="ignore"):
        s2 = r * r * dual2
        m2 = mu * mu
        up, down = pri2 > m2 * s2, s2 > m2 * pri2
        r_up, r_down = r * tau, r * tau_inv
        r_up = np.where(r_up < hi, r_up, hi)
        r_down = np.where(r_down > lo, r_down, lo)
    return np.where(up, r_up, np.where(down, r_down, r))


def step(w, sums, abl, mu, tau, lo=(RHO_MIN,) * 3, hi=(RHO_MAX,) * 3):
    """w: dict rho, rho_u, rho_d -> float64 array (B,) or float; sums: (NMETRIC, B) squares (a row of metrics_per_sample).
    Returns the dict after one step."""
    has_phi, has_zd = has(abl)
    out = dict(w)
    for f, (nm, ip, idd) in enumerate(PAIRS):
        if (nm == "rho" and not has_phi) or (nm == "rho_d" and not has_zd):
            continue
        out[nm] = balance(w[nm], sums[ip], sums[idd], mu, tau, lo[NAMES.index(nm)], hi[NAMES.index(nm)])
    return out


def steps_after(it, start, every, until=None):
    n = start + it + 1
    return n % every == 0 and (until is None or n <= until)


def adaptive_dict(every, mu, tau, until=None):
    return dict(every=every, mu=mu, tau=tau, until=until, rho_min=RHO_MIN, rho_max=RHO_MAX)


def twin_clamps(i):
    """(rho_min, rho_max) of case i's comparisons against the twin, each in the order rho, rho_u, rho_d."""
    f = TWIN_CLAMPS[has(CASES[i][1])[0]]
    return tuple([f[k][j] * float(info()[nm]) for k, nm in enumerate(NAMES[:3])] for j in (0, 1))


def twin_dict(i, every, mu, tau):
    """adaptive_rho of case i's comparisons against the twin."""
    lo, hi = twin_clamps(i)
    return dict(every=every, mu=mu, tau=tau, rho_min=lo, rho_max=hi)


# ------------------------------------------------------------------------------------------------ the float64 twin
def adaptive_oracle(mode, abl, every, mu, tau, start_w=None, until=None, start=0, clamps=None):
    """An OracleADMM whose rho, rho_u, rho_d are properties: in iteration k = len(self.hist.p_res_list) they return the start
    values with the rule applied after every iteration it < k that steps_after() names, on the squares of that iteration's
    residual norms (float64).  `o.ad_log`: per step (it, {name: value}), `o.ad_margins`: |log| distances of every decision's
    two comparisons from equality, in the norms; `o.ad_dirs`: +1 / -1 / 0 of every decision."""
    o = make_oracle(meta(), mode, ablation=abl)
    has_phi, has_zd = has(abl)
    w0 = {nm: float(info()[nm]) for nm in NAMES[:3]}
    w0.update(start_w or {})
    lo, hi = clamps or ([RHO_MIN] * 3, [RHO_MAX] * 3)
    cols = {"rho_u": 0, "rho": 1 if has_phi else None, "rho_d": (2 if has_phi else 1) if has_zd else None}

    def current(self):
        h = self.hist
        if getattr(self, "_ad_hist", None) is not h:
            self._ad_hist, self._ad_done, self._ad_w = h, 0, dict(w0)
            self.ad_log, self.ad_margins, self.ad_dirs = [(-1, dict(w0))], [], []
        k = len(h.p_res_list)
        while self._ad_done < k:
            it = self._ad_done
            self._ad_done += 1
            if not steps_after(it, start, every, until):
                continue
            for nm, col in cols.items():
                if col is None:
                    continue
                r = self._ad_w[nm]
                pri2, dual2 = np.float64(h.p_res_list[it][col]) ** 2, np.float64(h.d_res_list[it][col]) ** 2
                new = float(balance(r, pri2, dual2, mu, tau, lo[NAMES.index(nm)], hi[NAMES.index(nm)]))
                s2 = r * r * dual2
                with np.errstate(divide="ignore"):
                    d = 0.5 * np.log(pri2 / s2) if pri2 > 0 and s2 > 0 else np.inf
                self.ad_margins.append(float(min(abs(d - np.log(mu)), abs(d + np.log(mu)))))
                self.ad_dirs.append(int(np.sign(new - r)))
                self._ad_w[nm] = new
            self.ad_log.append((it, dict(self._ad_w)))
        return self._ad_w

    props = {}
    for nm in NAMES[:3]:
        props[nm] = property(lambda self, nm=nm: current(self)[nm], lambda self, v: None)
    o.__class__ = type("Adaptive" + type(o).__name__, (type(o),), props)
    return o


def twin_history(o):
    """(P, 3) rho, rho_u, rho_d by period as mgadmm_solver_get_adaptive_history orders them: row 0 the start values, a row per
    step the solve took (call after combined_loop; the step after the last iteration is taken here)."""
    _ = o.rho      # (brings the replay up to the iterations done)
    return np.array([[w["rho"], w["rho_u"], w["rho_d"]] for _, w in o.ad_log])


@functools.lru_cache(maxsize=None)
def twin_solutions(i, every, mu, tau, n_iters=K):
    """[(x (1, T, N, 1) float64, oracle)] of the 8 samples of case i."""
    mode, abl = CASES[i]
    y64 = inputs().double().numpy()
    out = []
    for b in range(y64.shape[0]):
        o = adaptive_oracle(mode, abl, every, mu, tau, clamps=twin_clamps(i))
        out.append((o.combined_loop(y64[b:b + 1], n_iters=n_iters), o))
        twin_history(o)
    return out


def constant_solutions(i, n_iters=K):
    return pc.constant_solutions(i, n_iters)


def case_report(i, every, mu, tau):
    """(smallest margin as a log, steps up, steps down) over the 8 samples of case i."""
    tw = [o for _, o in twin_solutions(i, every, mu, tau)]
    return (min(min(o.ad_margins) for o in tw), sum(d > 0 for o in tw for d in o.ad_dirs), sum(d < 0 for o in tw for d in o.ad_dirs))


@functools.lru_cache(maxsize=None)
def triple(i):
    """The first of CANDIDATES that meets both conditions in case i; RuntimeError when none does."""
    tried = {}
    for t in CANDIDATES:
        m, up, down = tried[t] = case_report(i, *t)
        if m >= np.log(1 + MARGIN) and up > 0 and down > 0:
            return t
    raise RuntimeError(f"no (every, mu, tau) of {CANDIDATES} keeps every decision of case {IDS[i]} {MARGIN:.0%} from its thresholds "
                       f"with steps in both directions: {tried}")
