"""Census of the k_admm_lds instances the library ships (csrc/lds_launch.hip): one row per instance, with a problem
that reaches it, and the graph builders those problems use.

Every row names the instance string `nm -C` prints for its kernel and the problem that makes the planner
(csrc/lds_plan.h) pick it: N, T, t_in, graph kind, the largest W_d^T in-degree of the graph, ablation, task and
batch.  tests/test_lds_census_cpu.py checks that the rows cover exactly the shipped instances and that the graphs have
the stated in-degrees; tests/test_gpu_lds_census.py runs every row against the float64 oracle and asserts the instance
the solver reports it ran (MGADMM_Q_LDS_INSTANCE).

Environment switches (`env`) are used only where no input reaches an instance by the planner's own choice:
  MGADMM_LDS_NOSLOTS  the four 640-thread TPG-12 instances without slots and with a compile-time tail (TP 0..3): every
                      graph of that class with a tail of at most 3 pairs has room for the slot vectors
  MGADMM_LDS_SB       the four single-buffer instances (an experiment switch; never chosen by the planner)
  MGADMM_LDS_TABLE_ORDER=1 on one row: table entry order instead of the bank-conflict search
Graph kinds:
  uniform   k = 4 table without pads (ring with neighbours +-1, +-2, entries redirected to a hub): uniform-row instances
  knn3      k = 3 table without pads (ring neighbours +-1 and the opposite node): generic instances
  knnpad    k = 4 ring plus a component of 3 nodes whose rows hold two neighbours and two -1 pads: generic instances
  physical  the padded physical adjacency of a PEMS-like graph (path + chords) with hub edges: generic instances
  line1 / line3  line graph (band mode), skip connection 1 / 3: generic band instances
"""
import numpy as np
import torch

NLEAD = 5           # W_d^T entries per row held in registers by k_admm_lds (csrc/lds_consts.h, LDS_NLEAD)


def inst(tpg, band, maxt, sb, nu=0, nd=0, slots=False, tp=-1):
    b = lambda v: "true" if v else "false"
    return f"k_admm_lds<{tpg}, {b(band)}, {maxt}, {b(sb)}, {nu}, {nd}, {b(slots)}, {tp}>"


def uni(tpg, maxt, slots, tp):
    return inst(tpg, False, maxt, False, 4, 5, slots, tp)


def tail_pairs(indeg):
    """Pairs of the padded W_d^T tail table for a largest off-diagonal in-degree `indeg` (csrc/lds_plan.h, tail_pairs)."""
    return (max(0, indeg - NLEAD) + 1) // 2


def row(expect, N, T, t_in, kind, indeg=None, abl="None", task="pred", B=3, env=None):
    return dict(expect=expect, N=N, T=T, t_in=t_in, kind=kind, indeg=indeg, abl=abl, task=task, B=B, env=env or {})


NOSLOTS = {"MGADMM_LDS_NOSLOTS": "1"}
SB = {"MGADMM_LDS_SB": "1"}

# Geometry of a row (planner's choice): G = T / TPG time groups, block = N * G rounded up to 64 threads, ghosts = block - N * G.
CENSUS = [
    # ---- uniform rows, TPG 8, 1024-thread class
    row(uni(8, 1024, True, 0), 341, 24, 12, "uniform", 5),                              # G 3, 1 ghost, t_in inside a group
    row(uni(8, 1024, True, 1), 43, 24, 16, "uniform", 6, "DGTV", "mask"),               # G 3, 63 ghosts
    row(uni(8, 1024, True, 2), 100, 16, 8, "uniform", 9, "DGLR", env={"MGADMM_LDS_TABLE_ORDER": "1"}),   # G 2
    row(uni(8, 1024, True, 3), 150, 48, 24, "uniform", 11, "UT"),                       # G 6, t_in on a group boundary
    row(uni(8, 1024, True, -1), 170, 48, 20, "uniform", 12, "None", "mask"),            # G 6
    row(uni(8, 1024, False, 0), 1000, 8, 4, "uniform", 5, B=70),                        # G 1, cluster order, B % 64 != 0
    row(uni(8, 1024, False, 1), 1024, 8, 6, "uniform", 7, "DGTV"),                      # G 1, 0 ghosts
    row(uni(8, 1024, False, 2), 500, 16, 8, "uniform", 9, "DGLR", "mask"),              # G 2
    row(uni(8, 1024, False, 3), 500, 16, 12, "uniform", 10),                            # G 2
    row(uni(8, 1024, False, -1), 1000, 8, 4, "uniform", 13, "UT"),                      # G 1, row stride TS = T (the padded one does not fit)
    # ---- uniform rows, TPG 12, 640-thread class
    row(uni(12, 640, True, 0), 180, 36, 12, "uniform", 5),                              # G 3
    row(uni(12, 640, True, 1), 577, 12, 6, "uniform", 6, "DGLR"),                       # G 1, 63 ghosts, cluster order
    row(uni(12, 640, True, 2), 200, 36, 18, "uniform", 9, "UT", "mask"),                # G 3
    row(uni(12, 640, True, 3), 600, 12, 6, "uniform", 11, "DGTV"),                      # G 1
    row(uni(12, 640, True, -1), 180, 36, 24, "uniform", 25),                            # G 3, long run-time tail
    row(uni(12, 640, False, 0), 575, 12, 6, "uniform", 5, "DGTV", env=NOSLOTS),         # G 1, 1 ghost
    row(uni(12, 640, False, 1), 200, 36, 12, "uniform", 7, "None", "mask", env=NOSLOTS),
    row(uni(12, 640, False, 2), 600, 12, 8, "uniform", 9, "UT", env=NOSLOTS),
    row(uni(12, 640, False, 3), 180, 36, 12, "uniform", 10, "DGLR", env=NOSLOTS),
    row(uni(12, 640, False, -1), 600, 12, 6, "uniform", 12),                            # G 1: the tail leaves no room for slots
    # ---- uniform rows, TPG 12, 1024-thread class (no slot instances)
    row(uni(12, 1024, False, 0), 400, 24, 12, "uniform", 5),                            # G 2
    row(uni(12, 1024, False, 1), 1000, 12, 6, "uniform", 7, "DGTV", "mask"),            # G 1, cluster order
    row(uni(12, 1024, False, 2), 300, 36, 12, "uniform", 9, "UT"),                      # G 3
    row(uni(12, 1024, False, 3), 200, 48, 24, "uniform", 11, "DGLR"),                   # G 4
    row(uni(12, 1024, False, -1), 512, 24, 12, "uniform", 12, B=5),                     # G 2, 0 ghosts
    # ---- generic instances (ragged rows / band mode)
    row(inst(1, False, 1024, False), 30, 24, 12, "knn3", abl="DGTV"),
    row(inst(1, True, 1024, False), 30, 24, 12, "line1", abl="UT"),
    row(inst(2, False, 1024, False), 60, 24, 12, "knnpad", task="mask"),
    row(inst(2, True, 1024, False), 60, 24, 12, "line3"),
    row(inst(3, False, 1024, False), 100, 24, 12, "physical", abl="DGLR"),
    row(inst(3, True, 1024, False), 100, 24, 12, "line1", abl="DGTV", task="mask"),
    row(inst(4, False, 1024, False), 150, 24, 12, "knn3"),
    row(inst(4, True, 1024, False), 150, 24, 12, "line3", abl="UT"),
    row(inst(6, False, 1024, False), 200, 24, 12, "physical", task="mask"),
    row(inst(6, True, 1024, False), 200, 24, 12, "line1"),
    row(inst(8, False, 1024, False), 307, 24, 12, "physical", abl="DGTV"),
    row(inst(8, True, 1024, False), 300, 24, 12, "line3", abl="DGLR"),
    row(inst(12, False, 640, False), 200, 36, 12, "knnpad", abl="UT"),
    row(inst(12, True, 640, False), 600, 12, 6, "line1"),
    row(inst(12, False, 1024, False), 400, 24, 12, "physical"),
    row(inst(12, True, 1024, False), 400, 24, 12, "line3", abl="DGTV"),
    # ---- single-buffer instances (MGADMM_LDS_SB)
    row(inst(12, False, 640, True), 180, 36, 12, "uniform", 8, env=SB),
    row(inst(12, True, 640, True), 600, 12, 6, "line1", abl="DGLR", env=SB),
    row(inst(8, False, 1024, True), 300, 24, 12, "knn3", abl="UT", task="mask", env=SB),
    row(inst(8, True, 1024, True), 400, 16, 8, "line3", env=SB),
]


# The planner's geometry for each row: (G, TS) = time groups per workgroup and LDS row stride in floats.  The GPU test asserts
# it through Q_LDS_THREADS (N * G), Q_LDS_ROWS (N + ghosts) and Q_LDS_ROW_STRIDE (TS); TS = T on the row whose padded
# stride does not fit.  Keys: the instance's template argument list.
GEOMETRY = {
    '<8, false, 1024, false, 4, 5, true, 0>': (3, 28),
    '<8, false, 1024, false, 4, 5, true, 1>': (3, 28),
    '<8, false, 1024, false, 4, 5, true, 2>': (2, 20),
    '<8, false, 1024, false, 4, 5, true, 3>': (6, 52),
    '<8, false, 1024, false, 4, 5, true, -1>': (6, 52),
    '<8, false, 1024, false, 4, 5, false, 0>': (1, 12),
    '<8, false, 1024, false, 4, 5, false, 1>': (1, 12),
    '<8, false, 1024, false, 4, 5, false, 2>': (2, 20),
    '<8, false, 1024, false, 4, 5, false, 3>': (2, 20),
    '<8, false, 1024, false, 4, 5, false, -1>': (1, 8),
    '<12, false, 640, false, 4, 5, true, 0>': (3, 36),
    '<12, false, 640, false, 4, 5, true, 1>': (1, 12),
    '<12, false, 640, false, 4, 5, true, 2>': (3, 36),
    '<12, false, 640, false, 4, 5, true, 3>': (1, 12),
    '<12, false, 640, false, 4, 5, true, -1>': (3, 36),
    '<12, false, 640, false, 4, 5, false, 0>': (1, 12),
    '<12, false, 640, false, 4, 5, false, 1>': (3, 36),
    '<12, false, 640, false, 4, 5, false, 2>': (1, 12),
    '<12, false, 640, false, 4, 5, false, 3>': (3, 36),
    '<12, false, 640, false, 4, 5, false, -1>': (1, 12),
    '<12, false, 1024, false, 4, 5, false, 0>': (2, 28),
    '<12, false, 1024, false, 4, 5, false, 1>': (1, 12),
    '<12, false, 1024, false, 4, 5, false, 2>': (3, 36),
    '<12, false, 1024, false, 4, 5, false, 3>': (4, 52),
    '<12, false, 1024, false, 4, 5, false, -1>': (2, 28),
    '<1, false, 1024, false, 0, 0, false, -1>': (24, 28),
    '<1, true, 1024, false, 0, 0, false, -1>': (24, 28),
    '<2, false, 1024, false, 0, 0, false, -1>': (12, 28),
    '<2, true, 1024, false, 0, 0, false, -1>': (12, 28),
    '<3, false, 1024, false, 0, 0, false, -1>': (8, 28),
    '<3, true, 1024, false, 0, 0, false, -1>': (8, 28),
    '<4, false, 1024, false, 0, 0, false, -1>': (6, 28),
    '<4, true, 1024, false, 0, 0, false, -1>': (6, 28),
    '<6, false, 1024, false, 0, 0, false, -1>': (4, 28),
    '<6, true, 1024, false, 0, 0, false, -1>': (4, 28),
    '<8, false, 1024, false, 0, 0, false, -1>': (3, 28),
    '<8, true, 1024, false, 0, 0, false, -1>': (3, 28),
    '<12, false, 640, false, 0, 0, false, -1>': (3, 36),
    '<12, true, 640, false, 0, 0, false, -1>': (1, 12),
    '<12, false, 1024, false, 0, 0, false, -1>': (2, 28),
    '<12, true, 1024, false, 0, 0, false, -1>': (2, 28),
    '<12, false, 640, true, 0, 0, false, -1>': (3, 36),
    '<12, true, 640, true, 0, 0, false, -1>': (1, 12),
    '<8, false, 1024, true, 0, 0, false, -1>': (3, 28),
    '<8, true, 1024, true, 0, 0, false, -1>': (2, 20),
}


def geometry(r):
    """(threads N * G, LDS rows N + ghosts, row stride TS, ghosts) the planner chooses for row r."""
    G, TS = GEOMETRY[r["expect"][len("k_admm_lds"):]]
    nth = r["N"] * G
    ghosts = (nth + 63) // 64 * 64 - nth
    return nth, r["N"] + ghosts, TS, ghosts


def row_id(r):
    return r["expect"].replace("k_admm_lds", "").replace(" ", "").replace("true", "T").replace("false", "F")


# ---------------------------------------------------------------------------------------------- graph builders
def _ring(N, k):
    offs = [1, -1, 2, -2][:k]
    i = np.arange(N)
    return np.stack([i] + [(i + o) % N for o in offs], 1).astype(np.int64)


def _distances(cl, seed):
    """Self 0, then strictly increasing positive distances along each row (pads: inf)."""
    rng = np.random.default_rng(seed)
    k = cl.shape[1] - 1
    dl = np.zeros(cl.shape, dtype=np.float32)
    dl[:, 1:] = np.cumsum(rng.uniform(20.0, 80.0, (cl.shape[0], k)), 1)
    dl[cl == -1] = np.inf
    return dl


def in_degrees(cl):
    """Off-diagonal W_d^T row lengths: how many other rows list each node."""
    nb = cl[:, 1:]
    own = np.arange(cl.shape[0])[:, None]
    keep = (nb != -1) & (nb != own)
    return np.bincount(nb[keep], minlength=cl.shape[0])


def uniform_tables(N, indeg, seed=0):
    """k = 4 tables (cl (N, 5) int64, dl (N, 5) float32) with no pad, whose largest W_d^T in-degree is `indeg` (>= 5),
    reached by one hub (node 0; from in-degree 6 on it is the only node above 4 but for at most three nodes of in-degree 5),
    and with a node of in-degree 0 (node N // 2, whose W_d^T row is padding only).

    A ring with neighbours +-1, +-2 (every in-degree 4); the four entries that list node N // 2 are redirected -- to the
    hub while it needs more, else to helper nodes (in-degree 5) -- and, for in-degrees above 8, entries of rows far from
    both are redirected to the hub."""
    assert indeg >= 5 and N >= 4 * indeg + 16
    cl = _ring(N, 4)
    hub, orphan = 0, N // 2
    deg = in_degrees(cl)
    need = indeg - deg[hub]
    helpers = iter(range(N // 4, N // 2 - 4))           # in-degree 4, away from the hub and the orphan
    for r in range(N):
        for c in range(1, 5):
            if cl[r, c] != orphan:
                continue
            if need > 0 and hub not in cl[r]:
                cl[r, c] = hub
                need -= 1
            else:
                h = next(helpers)
                while h in cl[r]:
                    h = next(helpers)
                cl[r, c] = h
    for r in range(N // 2 + 4, N - 4):                  # rows that list neither the hub nor the orphan
        if need == 0:
            break
        cl[r, 4] = hub
        need -= 1
    assert need == 0
    return torch.from_numpy(cl), torch.from_numpy(_distances(cl, seed))


def knn3_tables(N, seed=0):
    """k = 3 without pads, symmetric (N even): ring neighbours +-1 and the opposite node i + N / 2."""
    assert N % 2 == 0
    i = np.arange(N)
    cl = np.stack([i, (i + 1) % N, (i - 1) % N, (i + N // 2) % N], 1).astype(np.int64)
    return torch.from_numpy(cl), torch.from_numpy(_distances(cl, seed))


def knnpad_tables(N, seed=0):
    """k = 4 ring over nodes 0 .. N-4 plus a component of 3 nodes (N-3 .. N-1) whose rows hold the other two and two -1
    pads (what the reference's Dijkstra kNN gives a component smaller than k + 1)."""
    cl = _ring(N - 3, 4)
    small = np.array([[N - 3, N - 2, N - 1, -1, -1], [N - 2, N - 1, N - 3, -1, -1], [N - 1, N - 3, N - 2, -1, -1]])
    cl = np.concatenate([cl, small]).astype(np.int64)
    return torch.from_numpy(cl), torch.from_numpy(_distances(cl, seed))


def physical_graph(N, seed=0):
    """PEMS-like road graph (bench.pems_like_graph: path + chords) with hub edges: node 0 joined to 7 nodes, node N // 3
    to 5, so the padded rows of the physical adjacency range from 1 to 8+ neighbours within a wave."""
    import bench
    ue, ud = bench.pems_like_graph(N, int(round(N * 1.11)), seed=seed)
    have = set(map(tuple, ue.numpy().tolist()))
    extra = [(0, j) for j in range(N // 2, N // 2 + 7)] + [(N // 3, j) for j in range(N - 5, N)]
    extra = [e for e in extra if e not in have]
    rng = np.random.default_rng(seed)
    e = np.array(extra, dtype=np.int64)
    d = rng.uniform(3.0, 600.0, len(e))
    ue = torch.cat([ue, torch.from_numpy(e), torch.from_numpy(e[:, ::-1].copy())])
    ud = torch.cat([ud, torch.from_numpy(d), torch.from_numpy(d)])
    return ue, ud


def tables_for(r, seed=0):
    """(cl, dl) of a row's graph (None for the physical and line kinds, which the product builds itself)."""
    kind, N = r["kind"], r["N"]
    if kind == "uniform":
        return uniform_tables(N, r["indeg"], seed)
    if kind == "knn3":
        return knn3_tables(N, seed)
    if kind == "knnpad":
        return knnpad_tables(N, seed)
    if kind in ("line1", "line3"):                       # band mode: W_u from a k = 4 ring, the temporal edges are the band
        cl = _ring(N, 4)
        return torch.from_numpy(cl), torch.from_numpy(_distances(cl, seed))
    return None


# ------------------------------------------------------------------- census of the other two compilations of the instances
# The library compiles the instances three times: k_admm_lds (csrc/lds_launch.hip), k_admm_lds_ps with the per-sample stop test
# (lds_launch_ps.hip) and k_admm_lds_pp with per-sample weights (lds_launch_pp.hip).  tests/test_gpu_lds_census_units.py runs
# every census row through the last two and compares with the B = 1 solves of the first, bit for bit.  The constants and the
# tolerance picker of that test (plain numpy: tests/test_lds_census_cpu.py checks the picker on hand-made tables).
UNITS = ("ps", "pp")
UNIT_K = 12         # ADMM iterations of a row
UNIT_CHUNK = 4      # MGADMM_LDS_CHUNK of the batch solves: launch boundaries fall inside the K iterations
UNIT_MARGIN = 0.01  # no deciding residual within 1 % of the tolerance
# Rows that cannot meet the picker's conditions with K = 12 and the scales 0.5 + 1.5 b / (B - 1), {instance: dict(K=.., scales=..)}:
# their residuals fall by 6 .. 9 % per iteration from the third on, so a sample four times another does not come below the other's
# second residual within 12 iterations; with the scales 1 + b / (B - 1) (a factor of two) it does.
_NARROW = lambda B: 1.0 + np.arange(B) / (B - 1)
UNIT_OVERRIDES = {
    uni(8, 1024, False, 0): dict(scales=_NARROW(70)),
    uni(8, 1024, False, 1): dict(scales=_NARROW(3)),
    uni(8, 1024, False, -1): dict(scales=_NARROW(3)),
    uni(12, 640, True, 1): dict(scales=_NARROW(3)),
    uni(12, 640, False, -1): dict(scales=_NARROW(3)),
    inst(12, True, 640, True): dict(scales=_NARROW(3)),
}


def unit_k(r):
    return UNIT_OVERRIDES.get(r["expect"], {}).get("K", UNIT_K)


def unit_scales(r):
    """Factor of every sample's input: the samples converge at different iterations."""
    B = r["B"]
    s = UNIT_OVERRIDES.get(r["expect"], {}).get("scales")
    return 0.5 + 1.5 * np.arange(B) / (B - 1) if s is None else np.asarray(s, dtype=np.float64)


def unit_picks(r):
    return [0, r["B"] // 2, r["B"] - 1]


def stop_iterations(res, tol, K, chunk=UNIT_CHUNK, margin=UNIT_MARGIN):
    """First crossing n_b (iterations run, 1-based) of every row of `res` (picks, K) -- the residual that decides the stop test
    after each iteration -- under the tolerance `tol`.  Asserts what makes the tolerance a test of per-sample stopping:
    every n_b in [2, K - 1]; at least two distinct n_b; two picks stop in different launches of `chunk` iterations; no residual
    of a pick up to its n_b within `margin` of the tolerance (no stop is a rounding decision)."""
    res = np.asarray(res, dtype=np.float64)
    assert res.ndim == 2 and res.shape[1] == K and np.isfinite(res).all() and tol > 0, (res.shape, K, tol)
    n = []
    for b, row in enumerate(res):
        below = np.nonzero(row < tol)[0]
        assert below.size, f"pick {b} never falls below {tol!r} in {K} iterations"
        n.append(int(below[0]) + 1)
    assert all(2 <= v <= K - 1 for v in n), f"first crossings {n} not all in [2, {K - 1}] at {tol!r}"
    assert len(set(n)) >= 2, f"every pick stops at iteration {n[0]} at {tol!r}"
    assert len({-(-v // chunk) for v in n}) >= 2, f"first crossings {n}: every pick stops in the same launch of {chunk} at {tol!r}"
    for b, (row, v) in enumerate(zip(res, n)):
        near = np.abs(row[:v] / tol - 1.0) <= margin
        assert not near.any(), f"pick {b}: residual {row[:v][near][0]!r} of iteration {int(np.nonzero(near)[0][0]) + 1} within {margin} of {tol!r}"
    return n


def pick_admm_tol(res, K, chunk=UNIT_CHUNK, margin=UNIT_MARGIN):
    """(ADMM_tol, [n_b]) for a table `res` (picks, K) of deciding residuals: among the geometric means of neighbouring table
    values, the one that meets the conditions of stop_iterations with the most launches stopped in, then the most distinct
    n_b, then the widest gap to the nearest residual.  Raises AssertionError when no tolerance meets them."""
    res = np.asarray(res, dtype=np.float64)
    assert res.ndim == 2 and res.shape[1] == K and np.isfinite(res).all() and (res > 0).all(), (res.shape, K)
    vals = np.unique(res)
    best, why = None, "a table of one value"
    for tol in np.sqrt(vals[:-1] * vals[1:]):
        try:
            n = stop_iterations(res, tol, K, chunk, margin)
        except AssertionError as e:
            why = str(e)
            continue
        gap = min(float(np.abs(np.log(row[:v] / tol)).min()) for row, v in zip(res, n))
        score = (len({-(-v // chunk) for v in n}), len(set(n)), gap)
        if best is None or score > best[0]:
            best = (score, float(tol))
    assert best is not None, f"no tolerance meets the stop conditions (last candidate: {why})"
    return best[1], stop_iterations(res, best[1], K, chunk, margin)
