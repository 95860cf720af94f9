"""Census of the streaming path (k_rows, k_tile, k_cldr of csrc/stream_kernels.h; the dispatch rules in csrc/stream_plan.h, the
launch ladders that follow them in csrc/engine.h): one row per
PROBLEM, with the set of kernel instances the problem must launch.  tests/test_stream_census_cpu.py proves that the union of
the rows' sets plus the UNREACHABLE table is exactly what the built library ships; tests/test_gpu_stream_census.py runs every
row against the float64 oracle and asserts, through MGADMM_Q_STREAM_KEYS, that the named instances really ran.

The expected set of a row is not a recording: `expected(r)` restates the dispatch (streamplan::Planner of stream_plan.h: choose,
fused, fold1 / fold2, lu_fold_fits; the call sites of engine.h) from the row's dtype, batch, switches and the row lengths of
its three matrices, call by call of the phases the GPU test runs (operators, left-hand sides, CG solves, the ADMM loop).  The
GPU test asserts equality, so a change of the dispatch shows up as a named difference; tests/test_stream_plan_cpu.py compares
the planner itself with this model on the CPU."""
import os
import re

import numpy as np
import torch

import lds_census as lc
from conftest import PKG

# ------------------------------------------------------------------------------------------------------------ graphs
_OFFS = [1, -1, 2, -2, 3, -3, 4, -4]


def band_tables(N, k, hub_in=0, spread=1, ragged=False, seed=0):
    """Ring with the neighbours +-1, +-2, ... (k of them, k <= 8; odd k: and one far node): every W_d row has k + 1 entries (with the node itself)
    and every W_d^T row k + 1.  hub_in > k: node H = N // 3 is listed by hub_in rows -- the last entry of the rows
    H + k // 2 + 1 + j * spread is redirected to it -- so its W_d^T row has hub_in + 1 entries.  spread 1: the listing rows
    are neighbours of each other (a small 2-hop set); spread > k: their neighbourhoods are disjoint (a 2-hop set of about
    hub_in * k rows).  ragged: every 11th row ends in a -1 pad."""
    i = np.arange(N)
    cl = np.stack([i] + [(i + o) % N for o in _OFFS[:k - k % 2]], 1).astype(np.int64)
    if k % 2:
        # odd k: one more neighbour far away, paired (i <-> i + M / 2 over the first M = N or N - 1 nodes): like the others it is
        # listed in both directions, so that W_u stays symmetric (but for the last node of an odd N) and CG converges
        M = N - N % 2
        far = np.where(i < M, (i + M // 2) % M, (i + N // 2) % N)
        cl = np.concatenate([cl, far[:, None]], 1)
    if hub_in > k:
        H = N // 3
        for j in range(hub_in - k):
            r = (H + k // 2 + 1 + j * spread) % N
            assert H not in cl[r], (r, cl[r])
            cl[r, k] = H
    if ragged:
        cl[3::11, k] = -1
    return torch.from_numpy(cl), torch.from_numpy(lc._distances(cl, seed))


def scatter_tables(N, k, seed=0):
    """k random neighbours per node: no locality, a tile's rows name far more than TILE_HMAX = 20 out-of-tile rows."""
    rng = np.random.default_rng(seed + 17)
    cl = np.zeros((N, k + 1), dtype=np.int64)
    for i in range(N):
        cl[i, 0] = i
        cl[i, 1:] = rng.choice(np.delete(np.arange(N), i), k, replace=False)
    return torch.from_numpy(cl), torch.from_numpy(lc._distances(cl, seed))


def tables_for(r):
    """(cl, dl) of a row's graph; None for the physical kind (the product builds its adjacency from the edge list)."""
    g = r["graph"]
    kind = g[0]
    if kind == "band":
        return band_tables(r["N"], **g[1])
    if kind == "scatter":
        return scatter_tables(r["N"], **g[1])
    if kind in ("line", "skip3"):
        return band_tables(r["N"], 4)
    return None


def row_lengths(r):
    """(mu, md, mt, at): longest row of W_u, W_d, W_d^T and ceil(mean row length) of W_d^T, as the library counts them
    (graph.hip: W_u holds the k neighbours, W_d the node itself and its neighbours; -1 pads hold no entry; the physical
    graph applies W_d itself as the transpose)."""
    if r["graph"][0] == "physical":
        from mgadmm import utils
        ue, ud = lc.physical_graph(r["N"])
        cl = utils.connect_list(r["N"], ue, ud)[0].numpy()
    else:
        cl = tables_for(r)[0].numpy()
    N = cl.shape[0]
    lens = (cl[:, 1:] != -1).sum(1)
    if r["graph"][0] in ("line", "skip3"):
        return int(lens.max()), 0, 0, 0
    if r["graph"][0] == "physical":
        return int(lens.max()), int(lens.max()) + 1, int(lens.max()) + 1, -(-int(lens.sum() + N) // N)
    indeg = np.bincount(cl[:, 1:][cl[:, 1:] != -1], minlength=N) + 1
    return int(lens.max()), int(lens.max()) + 1, int(indeg.max()), -(-int(lens.sum() + N) // N)


# ------------------------------------------------------------------------- the dispatch of stream_plan.h and engine.h
def cldr_geoms():
    """{geometry: (VECT, NW, MA, MQ, MP)} read from CLDR_GEOMS in csrc/cldr_tiles.h, the table stream_plan.h reads and engine.h builds ClG1 ... ClG4 from."""
    hdr = open(os.path.join(PKG, "csrc", "cldr_tiles.h")).read()
    body = re.search(r"CLDR_GEOMS\[\d+\]\s*=\s*\{(.*?)\};", hdr, re.S).group(1)
    rows = re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\}", body)
    return {i: tuple(map(int, v)) for i, v in enumerate(rows) if i}


CLDR_GEOMS = cldr_geoms()
ABL_HAS_PHI = {"None": True, "DGLR": True, "DGTV": False, "UT": False}


def vec_of(dtype, B):
    """streamplan::Planner::make_geom: columns per lane and the padded batch."""
    if dtype == "f32":
        v = 4 if B >= 192 else 2 if B >= 96 else 1
    else:
        v = 2 if B >= 96 else 1
    return v, -(-B // (64 * v)) * 64 * v


class Dispatch:
    """The launches of a solver on row r, as names (`nm -C` spelling)."""

    def __init__(self, r, **override):
        r = dict(r, **override)
        env = r["env"]
        self.S = "float" if r["dtype"] == "f32" else "double"
        self.VEC, self.Bp = vec_of(r["dtype"], r["B"])
        self.mu, self.md, self.mt, self.at = row_lengths(r)
        self.spatial = r["graph"][0] not in ("line", "skip3")
        self.abl = r["abl"]
        flag = lambda k: env.get(k, "1") != "0"
        self.fold, self.fold_lu = flag("MGADMM_FOLD"), flag("MGADMM_FOLD_LU")
        self.tile = bool(r["reorder"]) and flag("MGADMM_TILE") and self.spatial                    # make_tile_geom
        self.MR = 5 if env.get("MGADMM_TILE_R") == "20" else 2
        self.geom = int(env.get("MGADMM_CLDR_GEOM", 1 if r["dtype"] == "f32" else 2))
        vect = CLDR_GEOMS[self.geom][0]
        # cldr_fits: the tables exist (r["slots"]: what MGADMM_Q_CLDR_SLOTS must report) and Bp is a multiple of the chunk width
        self.fused = self.tile and flag("MGADMM_FUSED") and r["slots"] > 0 and self.Bp % (64 * vect) == 0
        self.slots = r["slots"]
        self.out = set()

    # --- launch sites
    def rows(self, epi, op):
        """Planner::choose (launched by Engine::rows + rows_v).  op: 'none' | 'band' | 'lu' | 'ldr' | 'ldrt', '+self' for the operators of Ln (self_w set)."""
        S, V = self.S, self.VEC
        base, own_self = op.split("+")[0], op.endswith("+self")
        if not self.spatial and base in ("ldr", "ldrt"):
            base = "band"
        if base in ("lu", "ldr", "ldrt") and not own_self and self.tile:
            m = {"lu": self.mu, "ldr": self.md, "ldrt": self.mt}[base]
            tgw = 4 if m <= 4 else 8 if (base == "ldrt" or m > 6) else 6
            self.out.add(f"k_tile<{S}, {V}, {epi}<{S}, {V}>, {tgw}, {self.MR}, TileSrcPlain<{S}, {V}> >")
            return
        m = {"none": 0, "band": 0, "lu": self.mu, "ldr": self.md, "ldrt": self.at}[base]          # gather_width
        self.out.add(f"k_rows<{S}, {V}, {epi}<{S}, {V}>, {4 if m <= 4 else 6}>")

    def cldr(self, epi, src):
        S = self.S
        vect, nw, ma, mq, mp = CLDR_GEOMS[self.geom]
        minw = 2 if (self.geom == 2 and S == "double") else 4
        gd = 8 if self.md > 6 else 6
        self.out.add(f"k_cldr<{S}, {vect}, {epi}<{S}, {vect}>, CldrSrc{src}<{S}, {vect}>, {nw}, {ma}, {mq}, {mp}, {gd}, {self.slots}, {minw}>")

    # --- phases
    def kind(self, which):
        if which == "x":
            return 1 if ABL_HAS_PHI[self.abl] else 0
        return 2 if which == "zu" else 1

    def apply(self, op):
        if op in ("Lu", "Ldr", "Ldr_T"):
            self.rows("EpiStore", {"Lu": "lu", "Ldr": "ldr", "Ldr_T": "ldrt"}[op])
        elif op == "phi_direct":
            self.rows("EpiPhiDirect", "ldr")
        elif op == "cLdr":
            if self.fused:
                self.cldr("EpiStore", "Plain")
            else:
                self.rows("EpiStore", "ldr")
                self.rows("EpiStore", "ldrt")
        elif not self.spatial:                                   # Ln of the line graph
            self.rows("EpiLnLine", "none")
        else:
            self.rows("EpiStore", "ldr+self")
            self.rows("EpiAddTo", "ldrt+self")

    def lhs(self, which):
        k = self.kind(which)
        if k == 1 and self.fused:
            self.cldr("EpiLhs", "Plain")
        elif k == 1:
            self.rows("EpiStore", "ldr")
            self.rows("EpiLhs", "ldrt")
        else:
            self.rows("EpiLhs", "lu" if k == 2 else "none")

    def cg(self, which):
        k = self.kind(which)
        if k == 1 and self.fused:
            self.cldr("EpiCgInit", "Plain")
        elif k == 1:
            self.rows("EpiStore", "ldr")
            self.rows("EpiCgInit", "ldrt")
        else:
            self.rows("EpiCgInit", "lu" if k == 2 else "none")
        lu_fold_vec = 4 if self.S == "float" else 2
        fold2 = k == 2 and self.fold and self.fold_lu and self.tile and self.VEC == lu_fold_vec and self.mu <= 4 and self.MR == 2
        fold1 = k == 1 and self.fold and self.fused
        if fold2:
            S, V = self.S, self.VEC
            self.out.add(f"k_tile<{S}, {V}, EpiLhs<{S}, {V}>, 4, 2, TileSrcFold<{S}, {V}> >")
        elif fold1:
            self.cldr("EpiLhs", "Fold")
        else:
            self.lhs(which)
        self.rows("EpiCgUpdate", "none")
        self.rows("EpiXFinal" if (fold1 or fold2) else "EpiPUpdate", "none")

    def solve(self):
        has_phi, has_zd = ABL_HAS_PHI[self.abl], self.abl != "DGLR"
        if has_phi:
            self.rows("EpiStore", "ldr")                        # phi_0 = Ldr x_0
            self.rows("EpiLin2", "none")
            self.rows("EpiRhsX", "ldrt")
        else:
            self.rows("EpiRhsX", "none")
        self.cg("x")
        self.rows("EpiLin2", "none")
        self.cg("zu")
        if has_zd:
            self.cg("zd")
        self.rows("EpiDual", "none")
        self.rows("EpiPhi", "ldr")
        self.rows("EpiDot", "lu")


OPERATORS = ("Lu", "Ldr", "Ldr_T", "cLdr", "Ln", "phi_direct")


def lhs_list(r):
    return ("x", "zu") + (("zd",) if r["abl"] != "DGLR" else ())


def expected(r, phases=("ops", "cg", "cg_nofold", "solve"), **override):
    """Instances the phases of tests/test_gpu_stream_census.py launch on one solver of row r."""
    d = Dispatch(r, **override)
    if "ops" in phases:
        for op in OPERATORS:
            d.apply(op)
        for w in lhs_list(r):
            d.lhs(w)
    if "cg" in phases:
        for w in lhs_list(r):
            d.cg(w)
    if "solve" in phases:
        d.solve()
    return d.out


def expected_all(r):
    """... and on the second solver of the test, created under MGADMM_FOLD=0 for the CG solves."""
    return expected(r) | expected(r, phases=("cg",), env=dict(r["env"], MGADMM_FOLD="0"))


# ------------------------------------------------------------------------------------------------------------- rows
def row(name, N, T, graph, dtype, B, abl="None", task="pred", env=None, reorder=True, slots=0, tile_rows=None):
    env = dict(env or {})
    spatial = graph[0] not in ("line", "skip3")
    if tile_rows is None:
        tile_rows = 0 if not (reorder and spatial and env.get("MGADMM_TILE", "1") != "0") else (20 if env.get("MGADMM_TILE_R") == "20" else 8)
    return dict(name=name, N=N, T=T, t_in=T // 2, graph=graph, dtype=dtype, B=B, abl=abl, task=task, env=env, reorder=reorder,
                slots=slots, tile_rows=tile_rows)


def row_id(r):
    return r["name"]


ABLS = ("None", "DGTV", "DGLR", "UT")
TASKS = ("pred", "mask")
_SIZES = (96, 101, 131, 160)
CENSUS = []


def _cldr_rows():
    """k_cldr: every (scalar type, geometry, GD, GT) class; ablation and task rotate so that every ablation and the mask
    task occur under every float32 geometry and in float64."""
    n = 0
    for dtype, geoms in (("f32", (1, 2, 3, 4)), ("f64", (2,))):
        for geom in geoms:
            for gd in (6, 8):
                for gt in (12, 16, 24):
                    v = n % 2                 # two graphs per class, alternating: the other k, the row length at the class's upper end
                    k = {6: (4, 5), 8: (7, 6)}[gd][v]
                    hub_in = {12: (0, 11), 16: (13, 15), 24: (21, 23)}[gt][v]
                    B = {1: 256, 4: 256, 3: 100, 2: 70}[geom] if dtype == "f32" else (70, 100)[(n // 2) % 2]
                    env = {} if (dtype == "f32" and geom == 1) or dtype == "f64" else {"MGADMM_CLDR_GEOM": str(geom)}
                    CENSUS.append(row(f"cldr-{dtype}-g{geom}-gd{gd}-gt{gt}", _SIZES[n % 4], (4, 12)[n % 3 == 0],
                                      ("band", dict(k=k, hub_in=hub_in)), dtype, B, ABLS[(n + n // 4) % 4], TASKS[(n // 2) % 2], env, slots=gt))
                    n += 1
    # VEC 2 under the 256-column geometry (Bp = 256), and two column chunks in both dispatch orders
    CENSUS.append(row("cldr-f32-g1-B130", 131, 4, ("band", dict(k=4)), "f32", 130, "None", "mask", slots=12))
    for order in ("1", "0"):
        CENSUS.append(row(f"cldr-f32-g1-B300-order{order}", 101, 4, ("band", dict(k=6, hub_in=13)), "f32", 300, "DGLR", "pred",
                          {"MGADMM_CLDR_ORDER": order}, slots=16))


def _tile_rows():
    """k_tile: every (scalar type, VEC, TILE_GW, MR) class with the two-pass operators (MGADMM_FUSED=0: the fused kernel
    would take Ldr^T Ldr away from k_tile).  TILE_GW 4: k = 2 (every row of the three matrices has at most 4 entries) and
    k = 3; 6: k = 5; 8: k = 7, with a hub (overflow by row length) or scattered neighbours (overflow by halo capacity)."""
    n = 0
    for dtype, Bs in (("f32", (3, 100, 256)), ("f64", (3, 100))):
        for B in Bs:
            for tile_r in (None, "20"):
                for tgw, graph in ((4, ("band", dict(k=2))), (6, ("band", dict(k=5, ragged=True))),
                                   (8, ("scatter", dict(k=7)) if (n // 3) % 4 in (0, 3) else ("band", dict(k=7, hub_in=13)))):
                    env = {"MGADMM_FUSED": "0"}
                    if tile_r:
                        env["MGADMM_TILE_R"] = tile_r
                    # (EpiRhsX runs with W_d^T only where the ablation has phi: 'None' / 'DGLR')
                    CENSUS.append(row(f"tile-{dtype}-B{B}-gw{tgw}-r{tile_r or 8}", (101, 131, 100, 157)[n % 4], (4, 12)[n % 5 == 0], graph, dtype, B,
                                      ("None", "DGLR")[(n // 3) % 2], TASKS[n % 2], env))
                    n += 1
    # k = 3: W_u and W_d rows in 4 slots, W_d^T rows in 8; N < R for both tile sizes
    CENSUS.append(row("tile-f32-B256-k3", 131, 4, ("band", dict(k=3)), "f32", 256, "None", "mask", {"MGADMM_FUSED": "0"}))
    CENSUS.append(row("tile-f64-B100-k3", 100, 4, ("band", dict(k=3)), "f64", 100, "UT", "pred", {"MGADMM_FUSED": "0"}))
    CENSUS.append(row("tile-f32-B3-N7", 7, 4, ("band", dict(k=2)), "f32", 3, "None", "pred", {"MGADMM_FUSED": "0"}))
    CENSUS.append(row("tile-f64-B3-N13-r20", 13, 4, ("band", dict(k=5)), "f64", 3, "None", "mask", {"MGADMM_FUSED": "0", "MGADMM_TILE_R": "20"}))


def _rows_rows():
    """k_rows: every (scalar type, VEC, GW) class in the natural node order: kNN with k = 3 and k = 6, the physical graph
    with its padded rows, and the two line graphs (band operators, EpiLnLine)."""
    n = 0
    for dtype, Bs in (("f32", (3, 100, 256)), ("f64", (3, 100))):
        for B in Bs:
            for k in (3, 6):
                abl = ("DGTV", "UT")[(n // 2) % 2] if k == 3 else ("None", "DGLR")[(n // 2) % 2]      # (the wide EpiRhsX needs phi)
                CENSUS.append(row(f"rows-{dtype}-B{B}-k{k}", (96, 131)[n % 2], (4, 12)[n % 4 == 0], ("band", dict(k=k, ragged=k == 6)), dtype, B,
                                  abl, TASKS[(n // 2 + n) % 2], reorder=False))
                n += 1
    for dtype, B, kind in (("f32", 256, "physical"), ("f64", 100, "physical"), ("f32", 100, "line"), ("f64", 3, "line"), ("f32", 3, "line"),
                           ("f32", 256, "skip3"), ("f64", 100, "skip3")):
        CENSUS.append(row(f"rows-{dtype}-B{B}-{kind}", 101, 4 if kind == "line" else 12, (kind,), dtype, B, ABLS[n % 4], TASKS[n % 2], reorder=False))
        n += 1


def _fallback_rows():
    """Problems the fused kernel cannot take: the two-pass form runs, correct against the oracle, MGADMM_Q_CLDR_SLOTS 0."""
    CENSUS.append(row("fallback-k8", 131, 4, ("band", dict(k=8)), "f32", 256, "None", "pred"))                         # W_d rows of 9 entries
    CENSUS.append(row("fallback-hub25", 160, 4, ("band", dict(k=6, hub_in=24)), "f32", 256, "None", "mask"))            # a W_d^T row of 25
    CENSUS.append(row("fallback-c2cap", 160, 4, ("band", dict(k=4, hub_in=20, spread=6)), "f32", 256, "None", "pred"))   # 2-hop set > 40 rows
    CENSUS.append(row("fallback-B70-g1", 101, 4, ("band", dict(k=4)), "f32", 70, "None", "mask"))                       # Bp = 128 under 256-column chunks
    CENSUS.append(row("fallback-fused0", 101, 4, ("band", dict(k=4)), "f32", 256, "DGTV", "pred", {"MGADMM_FUSED": "0"}))
    CENSUS.append(row("fallback-f64-k8", 96, 4, ("band", dict(k=8)), "f64", 100, "None", "pred"))


_cldr_rows()
_tile_rows()
_rows_rows()
_fallback_rows()
assert len({r["name"] for r in CENSUS}) == len(CENSUS)

# ------------------------------------------------------------------------------------------------------ unreachable
# Shipped instances no problem can launch: (regular expression, "<file> <function>: the dispatch line there that excludes them").
# The CPU test requires every shipped name to be in a row's set or to match exactly one of these, every pattern to match
# something, and the named function to stand in the named file.
UNREACHABLE = [
    (r"k_tile<.*, EpiAddTo<.*",
     "engine.h op_ln: EpiAddTo runs with the father operator of Ln only, whose self_w is set; Planner::choose (stream_plan.h) takes "
     "k_tile only for an operator without self_w, so Ln always runs k_rows"),
    (r"k_tile<.*, EpiRhsX<[^>]*>, 6, .*",
     "engine.h admm_step: the spatial EpiRhsX launch applies op_ldrt (W_d^T); Planner::choose (stream_plan.h) gives W_d^T 4 or 8 "
     "slots, never 6"),
    (r"k_rows<.*, Epi(CgUpdate|PUpdate|XFinal|Lin2|Dual|LnLine)<[^>]*>, 6>",
     "stream_plan.h choose: the element-wise epilogues run with op_none (no spatial matrix): gather window 4"),
]
