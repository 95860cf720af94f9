"""The common problem of the per-sample band-weight tests (tests/test_gpu_band_sets.py, tests/test_band_sets_cpu.py): the
smallest on which each kernel can still go wrong.  Plain builders, no device needed.

  graph    the 30-node graph of g4_meta.npz, T = 24, t_in = 12, a line-graph instance of width WIDTH = 6;
  sets     five: the uniform skip-connection intervals 1, 2, 3, 6 (rows 1 / min(t, s), zero beyond) and a decaying table
           0.5^s, row-normalised in float32 over the hops a row reads;
  windows  the fixture's window scaled by factors spread over [0.7, 1.3]; five consecutive samples share a window, so every
           window meets all five sets;
  sets of the samples   set_of_sample[b] = (3 b + b // 64) % 5: neighbouring lanes, the lanes of one vector and the two sides
           of a 64-column boundary all differ.

The float64 oracle's solutions of one window under two different sets differ by 1.4e-3 ... 7e-3 relative on the predicted
steps (3 and 6 iterations, all three ablations: min_set_difference), at least 140 x the float32 tolerance of 1e-5; the
oracle run with a zero-padded table and with the native width agree exactly."""
import functools
import itertools

import numpy as np
import torch

from conftest import admm_info_from, load_golden

WIDTH = 6
INTERVALS = (1, 2, 3, 6)                  # sets 0 .. 3; set 4: the decaying table
N_SETS = 5
ABLATIONS = ("None", "DGLR", "DGTV")
F32_TOL = dict(xtol=1e-5, htol=1e-3, slack=1)         # tests/test_gpu_random.py:80-81
F64_TOL = dict(xtol=1e-9, htol=1e-7, slack=0)


def meta():
    return load_golden("g4_meta.npz")


def dims():
    m = meta()
    return int(m["T"]), int(m["t_in"]), int(m["n"])


def uniform_table(s, width=WIDTH):
    """(T, width) float32: rows 1 / min(t, s) on the hops h < min(t, s), zero beyond -- skip-connection interval s."""
    T = dims()[0]
    w = np.zeros((T, width), dtype=np.float32)
    for t in range(1, T):
        m = min(t, s)
        w[t, :m] = np.float32(1.0) / np.float32(m)
    return w


def decaying_table():
    """(T, WIDTH) float32: 0.5^h on the hops a row reads, row-normalised in float32."""
    T = dims()[0]
    w = np.zeros((T, WIDTH), dtype=np.float32)
    for t in range(1, T):
        m = min(t, WIDTH)
        row = np.float32(0.5) ** np.arange(m, dtype=np.float32)
        w[t, :m] = row / row.sum(dtype=np.float32)
    return w


def tables():
    """The five sets in the instance's width: a list of (T, WIDTH) float32 arrays."""
    return [uniform_table(s) for s in INTERVALS] + [decaying_table()]


def set_of_sample(B):
    b = np.arange(B)
    return ((3 * b + b // 64) % N_SETS).astype(np.int32)


def window_of_sample(B):
    return np.arange(B) // N_SETS


def factors(B):
    nw = int(window_of_sample(B)[-1]) + 1
    return np.ones(1) if nw == 1 else 0.7 + 0.6 * np.arange(nw) / (nw - 1)


def inputs(B, task="pred", dtype=np.float32):
    """(y, mask) of B samples as torch tensors: prediction (B, t_in, N, 1) / None, or the mask task (B, T, N, 1) twice."""
    m = meta()
    t_in = dims()[1]
    x = m["x_true"].astype(np.float64) * factors(B)[window_of_sample(B)].reshape(B, 1, 1, 1)
    if task == "pred":
        return torch.from_numpy(x[:, :t_in].astype(dtype)), None
    mask = np.broadcast_to(m["mask"].astype(np.float64), x.shape)
    return torch.from_numpy((x * mask).astype(dtype)), torch.from_numpy(mask.astype(dtype))


def instance(abl, skip=WIDTH, table=None, **kw):
    """A line-graph instance of the fixture's graph with skip_connection = skip; `table` (T, skip) overwrites its d_ew."""
    from mgadmm.ADMM import ADMM_algorithm
    m = meta()
    T, t_in, n = dims()
    tabs = (torch.from_numpy(m["knn_cl"]), torch.from_numpy(m["knn_dl"]))
    blk = ADMM_algorithm({"n_nodes": n}, admm_info_from(m), use_kNN=True, k=int(m["k"]), tables=tabs, u_sigma=float(m["sigma"]),
                         ablation=abl, t_in=t_in, T=T, use_line_graph=True, skip_connection=skip, **kw)
    # the fixture's own W_u (as helpers.make_product injects it): `exp` leaves last bits that depend on the CPU's vector units,
    # and the float64 comparison with the oracle, which reads the fixture's table, resolves them
    blk.u_ew = torch.from_numpy(np.asarray(m["knn_u_ew"], dtype=np.float32)).unsqueeze(0).repeat(T, 1, 1)
    if table is not None:
        blk.d_ew = torch.from_numpy(np.ascontiguousarray(table))[:, :, None].repeat(1, 1, n)
    return blk


def twin(abl, j, **kw):
    """The instance whose own graph is set j: skip_connection = the interval at its native width; the decaying set on a
    width-6 instance whose d_ew is overwritten."""
    return instance(abl, INTERVALS[j], **kw) if j < len(INTERVALS) else instance(abl, WIDTH, table=decaying_table(), **kw)


def oracle(abl, table, info=None, u_ew=None):
    """The float64 oracle on the fixture's graph with the band table `table` (T, skip) as its wt."""
    from oracle import admm_oracle as orc
    m = meta()
    T, t_in, _ = dims()
    o = orc.OracleADMM(m["knn_cl"], m["knn_u_ew"] if u_ew is None else u_ew, None, admm_info_from(m) if info is None else info,
                       mode="line", ablation=abl, t_in=t_in, T=T, skip_connection=table.shape[1])
    o.wt = np.asarray(table, dtype=np.float32)
    return o


@functools.lru_cache(maxsize=None)
def oracle_solutions(abl, n_iters, task="pred", n_windows=3):
    """(sets, windows, T, N, 1) float64: the oracle's x of every window of a B = 5 n_windows batch under every set."""
    B = N_SETS * n_windows
    y, mask = inputs(B, task, np.float64)
    first = np.arange(n_windows) * N_SETS                    # one sample of every window
    y64, m64 = y.numpy()[first], None if mask is None else mask.numpy()[first]
    return np.stack([oracle(abl, t).combined_loop(y64, mask=m64, n_iters=n_iters) for t in tables()])


def min_set_difference(abl, n_iters, task="pred"):
    """Smallest relative difference, on the predicted steps, between the oracle's solutions of one window under two sets."""
    xs = oracle_solutions(abl, n_iters, task)[:, :, dims()[1]:]
    worst = np.inf
    for a, b in itertools.combinations(range(xs.shape[0]), 2):
        d = np.linalg.norm((xs[a] - xs[b]).reshape(xs.shape[1], -1), axis=1) / np.linalg.norm(xs[b].reshape(xs.shape[1], -1), axis=1)
        worst = min(worst, float(d.min()))
    return worst


def predicted_difference(x, b0, b1):
    """Relative difference of two samples of a batch result on the predicted steps."""
    t_in = dims()[1]
    a, b = x[b0, t_in:].double(), x[b1, t_in:].double()
    return float((a - b).norm() / b.norm())
