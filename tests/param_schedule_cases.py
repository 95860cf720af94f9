"""Problems of the per-iteration weight tests (tests/test_gpu_param_schedule.py, tests/test_param_schedule_cpu.py): the
fixture of test_gpu_sample_params.py (tables of g4_meta.npz, N = 30, T = 24; the 8 inputs of g5_batched.npz; four cases), a
schedule table of 12 rows for K = 20 iterations -- the clamp to the last row and the launch boundary 16 + 4 are both hit --
and the float64 twin: the oracle with the six weights turned into properties of the iteration number.  Plain builders, no
device needed.

Sample b ramps rho, rho_u and rho_d together by TAU[b] ** row; samples 5 and 6 instead vary the mus linearly over the rows,
in multiples of the fixture's values: mu_u 0.5 -> 2, mu_d1 2 -> 0.5, mu_d2 1 -> 3.  Sample 0 (TAU = 1) has equal rows.

Measured on the CPU with this table over the 4 cases x 8 samples (test_param_schedule_cpu.py asserts the margins): the
twin's solution differs from the constant-weight solution by >= 1.2e-2 and from the same schedule shifted by one row by
>= 1.05e-3 (sample 0: exactly 0); no CG solve comes near the limit of 100 (the largest count is 25)."""
import functools

import numpy as np
import torch

from conftest import admm_info_from, load_golden
from helpers import make_oracle

NAMES = ("rho", "rho_u", "rho_d", "mu_u", "mu_d1", "mu_d2")
CASES = [("knn", "None"), ("knn", "DGLR"), ("line", "None"), ("physical", "DGTV")]      # those of test_gpu_sample_params.py
IDS = [f"{m}-{a}" for m, a in CASES]
N_ROWS, K = 12, 20
TAU = (1.0, 1.05, 1.1, 1.2, 0.95, 1.1, 1.0, 1.15)
MU_SAMPLES = (5, 6)
MU_RANGE = {"mu_u": (0.5, 2.0), "mu_d1": (2.0, 0.5), "mu_d2": (1.0, 3.0)}
F32_X_TOL = 1e-5          # the agreement test_gpu_parity.py demands of float32 solves against the float64 oracle
F32_HIST_RTOL = 1e-3


def meta():
    return load_golden("g4_meta.npz")


def inputs():
    return torch.from_numpy(load_golden("g5_batched.npz")["y"].astype(np.float32))


def info():
    return admm_info_from(meta())


def table(n_rows=N_ROWS, tau=TAU):
    """The per-sample form: dict name -> float64 array (n_rows, len(tau)); all six names, so that a column is a complete
    set of weights per row."""
    inf = info()
    B = len(tau)
    out = {nm: np.full((n_rows, B), float(inf[nm])) for nm in NAMES}
    rows = np.arange(n_rows, dtype=np.float64)
    for b, t in enumerate(tau):
        if b in MU_SAMPLES:
            for nm, (lo, hi) in MU_RANGE.items():
                out[nm][:, b] = float(inf[nm]) * np.linspace(lo, hi, n_rows)
        else:
            for nm in NAMES[:3]:
                out[nm][:, b] = float(inf[nm]) * float(t) ** rows
    return out


def column(tab, b):
    """The shared form of sample b's column: dict name -> (n_rows,)."""
    return {nm: np.ascontiguousarray(v[:, b]) for nm, v in tab.items()}


def padded(tab, n_rows):
    """The table padded by hand with copies of its last row."""
    return {nm: np.concatenate([v, np.repeat(v[-1:], n_rows - v.shape[0], 0)]) for nm, v in tab.items()}


def row_of(it, first_row, n_rows):
    return min(first_row + it, n_rows - 1)


def scalars_of(tab, b, it, first_row=0):
    """The six doubles sample b solves iteration `it` with."""
    n = next(iter(tab.values())).shape[0]
    return {nm: float(v[row_of(it, first_row, n), b]) for nm, v in tab.items()}


def scheduled_oracle(mode, abl, sched, first_row=0):
    """The float64 twin: an OracleADMM whose six weights are properties returning row min(first_row + k, n - 1) of `sched`
    (dict name -> 1-D array) in iteration k.  k = len(self.hist.p_res_list): combined_loop installs a fresh History and
    appends to p_res_list as the last thing an iteration does, after every use of a weight.  The setters ignore the
    constructor's setattr."""
    o = make_oracle(meta(), mode, ablation=abl)
    props = {}
    for nm, arr in sched.items():
        arr = np.asarray(arr, dtype=np.float64)
        assert nm in NAMES and arr.ndim == 1

        def get(self, arr=arr):
            return float(arr[min(first_row + len(self.hist.p_res_list), len(arr) - 1)])
        props[nm] = property(get, lambda self, v: None)
    o.__class__ = type("Scheduled" + type(o).__name__, (type(o),), props)
    return o


@functools.lru_cache(maxsize=None)
def twin_solutions(i, first_row=0, n_iters=K):
    """[(x (1, T, N, 1) float64, oracle)] of the 8 samples under their columns, case i."""
    mode, abl = CASES[i]
    y64, tab = inputs().double().numpy(), table()
    out = []
    for b in range(len(TAU)):
        o = scheduled_oracle(mode, abl, column(tab, b), first_row)
        out.append((o.combined_loop(y64[b:b + 1], n_iters=n_iters), o))
    return out


@functools.lru_cache(maxsize=None)
def constant_solutions(i, n_iters=K):
    mode, abl = CASES[i]
    y64 = inputs().double().numpy()
    return make_oracle(meta(), mode, ablation=abl).combined_loop(y64, n_iters=n_iters)
