"""Problems of the per-sample graph-weight tests (tests/test_gpu_graph_sets.py, tests/test_lds_graph_sets_cpu.py): the N = 30
graphs of g4_meta.npz with their distances, instances CONSTRUCTED with a pair (u_sigma, d_sigma), and the float64 oracle on
such an instance's tables.  Plain builders, no device needed.

PAIRS: four sigma pairs, both sigmas {0.5, 1, 2, 4} x the fixture's sigma (50).  Already at these factors the oracle's
solutions of any two pairs, on every one of the 8 inputs of g5_batched.npz and in every case of CASES that has spatial W_d
tables, differ by far more than 100 x the 1e-5 bound of a float32 solve (min_pair_difference: knn-None 0.128, knn-DGLR
0.137, physical-DGTV 0.115 after 40 iterations), so the factors were not widened: a kernel that reads the weights of another
set cannot pass the comparison with the oracle."""
import functools
import itertools

import numpy as np
import torch

from conftest import admm_info_from, load_golden

FACTORS = ((0.5, 0.5), (1.0, 1.0), (2.0, 2.0), (4.0, 4.0))      # (u_sigma, d_sigma) / sigma of the fixture
CASES = [("knn", "None"), ("knn", "DGLR"), ("line", "None"), ("physical", "DGTV")]      # those of test_gpu_sample_params.py
IDS = [f"{m}-{a}" for m, a in CASES]
FIXED_IT = 40
F32_X_TOL = 1e-5
MIN_DIFFERENCE = 100 * F32_X_TOL


def meta():
    return load_golden("g4_meta.npz")


def inputs():
    return torch.from_numpy(load_golden("g5_batched.npz")["y"].astype(np.float32))


def pairs(factors=FACTORS):
    s = float(meta()["sigma"])
    return [(fu * s, fd * s) for fu, fd in factors]


def instance(mode, abl, u_sigma, d_sigma, **kw):
    """ADMM_algorithm of the fixture's graph constructed with the pair: 'knn' / 'line' from the kNN tables and their distances,
    'physical' from the edge list (transpose_by_gather)."""
    from mgadmm.ADMM import ADMM_algorithm
    m = meta()
    common = dict(u_sigma=u_sigma, d_sigma=d_sigma, ablation=abl, t_in=int(m["t_in"]), T=int(m["T"]), **kw)
    if mode == "physical":
        e, d = torch.from_numpy(m["edges"]), torch.from_numpy(m["dist"])          # both directions, as utils.physical_graph lists them
        gi = {"n_nodes": int(m["n"]), "u_edges": torch.cat([e, e.flip(1)]), "u_dist": torch.cat([d, d])}
        return ADMM_algorithm(gi, admm_info_from(m), use_kNN=False, **common)
    tables = (torch.from_numpy(m["knn_cl"]), torch.from_numpy(m["knn_dl"]))
    return ADMM_algorithm({"n_nodes": int(m["n"])}, admm_info_from(m), use_kNN=True, k=int(m["k"]), tables=tables,
                          use_line_graph=mode == "line", **common)


def oracle_on(blk, mode, abl, info=None):
    """The float64 oracle on the tables `blk` holds (an instance constructed with a pair)."""
    from oracle import admm_oracle as orc
    m = meta()
    info = admm_info_from(m) if info is None else info
    return orc.OracleADMM(blk.connect_list.numpy(), blk.u_ew[0].numpy(), blk.d_ew[0].numpy(), info, mode=mode, ablation=abl,
                          t_in=int(m["t_in"]), T=int(m["T"]))


@functools.lru_cache(maxsize=None)
def oracle_solutions(i, n_iters=FIXED_IT):
    """(sets, 8, T, N, 1) float64: the oracle's x after n_iters iterations of every input under every pair, case i."""
    mode, abl = CASES[i]
    y64 = inputs().double().numpy()
    out = []
    for us, ds in pairs():
        o = oracle_on(instance(mode, abl, us, ds), mode, abl)
        out.append(o.combined_loop(y64, n_iters=n_iters))
    return np.stack(out)


def min_pair_difference(i):
    """Smallest relative difference between the oracle's solutions of one input under two different pairs."""
    xs = oracle_solutions(i)
    worst = np.inf
    for a, b in itertools.combinations(range(xs.shape[0]), 2):
        d = np.linalg.norm((xs[a] - xs[b]).reshape(xs.shape[1], -1), axis=1) / np.linalg.norm(xs[b].reshape(xs.shape[1], -1), axis=1)
        worst = min(worst, float(d.min()))
    return worst
