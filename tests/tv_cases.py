"""Shared builders of the time-varying tests: the problem of tests/golden/g11_time_varying.npz as a float64 restatement
(tests/tv_oracle.py) and as a product instance with ``time_varying=True``."""
import functools

import numpy as np
import torch

from conftest import load_golden
from tv_oracle import TvOracleADMM

INFO_KEYS = ("rho", "rho_u", "rho_d", "mu_u", "mu_d1", "mu_d2")


@functools.lru_cache(maxsize=None)
def g11():
    return load_golden("g11_time_varying.npz")


def info_ops():
    return {k: float(g11()["ops/" + k]) for k in INFO_KEYS}


def info_solve():
    return {k: float(load_golden("g4_meta.npz")[k]) for k in INFO_KEYS}


def tables(mode, T):
    """(cl, u_ew (T, N, k), d_ew (T-1, N, k+1)): the first slices of the fixture's tables."""
    g = g11()
    return g[mode + "_cl"], g[mode + "_u_ew"][:T], g[mode + "_d_ew"][:T - 1]


def make_tv_oracle(mode, T, t_in, info, **kw):
    cl, u, d = tables(mode, T)
    return TvOracleADMM(cl, u, d, info, mode=mode, t_in=t_in, T=T, **kw)


def make_tv_product(mode, T, t_in, info, u_ew=None, d_ew=None, time_varying=True, **kw):
    """mgadmm.ADMM_algorithm on the fixture's graph with the tables injected as make_product (tests/helpers.py) does."""
    from mgadmm.ADMM import ADMM_algorithm
    cl, u, d = tables(mode, T)
    u, d = (u if u_ew is None else u_ew), (d if d_ew is None else d_ew)
    clt = torch.from_numpy(cl)
    blk = ADMM_algorithm({"n_nodes": cl.shape[0]}, info, use_kNN=(mode == "knn"), k=cl.shape[1] - 1, u_sigma=1.0, d_sigma=1.0,
                         t_in=t_in, T=T, tables=(clt, torch.zeros(cl.shape) + 1.0), time_varying=time_varying, **kw)
    blk.u_ew = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32))
    blk.d_ew = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32))
    return blk


def row_lengths(mode):
    """Longest / shortest rows of W_u, W_d and W_d^T (the matrix Ldr_T gathers with) of the fixture's graph."""
    cl = g11()[mode + "_cl"]
    lu, ld = (cl[:, 1:] != -1).sum(1), (cl != -1).sum(1)
    lt = np.bincount(cl[cl != -1], minlength=cl.shape[0]) if mode == "knn" else ld
    return lu, ld, lt
