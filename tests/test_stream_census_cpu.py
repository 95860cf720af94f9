"""CPU checks of the streaming-path census (tests/stream_census.py): the rows' expected sets plus the UNREACHABLE table are
exactly the k_rows / k_tile / k_cldr instances the built library ships; the census graphs have the row lengths and in-degrees
the rows' classes need; the fused kernel's tile builder takes or refuses every census graph as the row states (the extended
tests/cpu/cldr_tiles_check.cpp on the graph itself); the key decoder and the query items agree with the headers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import stream_census as sc
from conftest import PKG, ROOT

LIB = os.path.join(PKG, "mgadmm", "libmgadmm.so")
SHIPPED = {"k_rows": 140, "k_tile": 242, "k_cldr": 120}


def shipped_instances():
    """Names of the streaming-kernel instances compiled into the library (one host launch stub per instance)."""
    if shutil.which("nm"):
        cmd = ["nm", "-C", LIB]
    else:
        cmd = [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump"), "--syms", "--demangle", LIB]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    names = set(re.findall(r"__device_stub__(k_(?:rows|tile|cldr)<.*>)\(", out))
    return {n.replace(">>", "> >") for n in names}


@pytest.fixture(scope="module")
def union():
    u = set()
    for r in sc.CENSUS:
        u |= sc.expected_all(r)
    return u


def test_census_and_unreachable_are_exactly_what_the_library_ships(union):
    shipped = shipped_instances()
    assert {k: sum(n.startswith(k + "<") for n in shipped) for k in SHIPPED} == SHIPPED
    excluded = {}
    for pat, why in sc.UNREACHABLE:
        where = re.match(r"(\w+\.h) (\w+): \S", why)                   # every entry names the file and the function of the dispatch line that excludes it
        assert where, pat
        assert re.search(r"\b%s\(" % where.group(2), open(os.path.join(PKG, "csrc", where.group(1))).read()), (pat, where.groups())
        hit = {n for n in shipped if re.fullmatch(pat, n)}
        assert hit, ("stale UNREACHABLE pattern", pat)
        assert not (hit & set(excluded)), ("two UNREACHABLE patterns for one instance", pat)
        excluded.update({n: pat for n in hit})
    assert not (union & set(excluded)), ("a census row expects an UNREACHABLE instance", sorted(union & set(excluded)))
    assert union | set(excluded) == shipped, dict(missing=sorted(shipped - union - set(excluded)), stale=sorted(union - shipped))
    print(f"\n[stream census] {len(shipped)} shipped = {len(union)} in {len(sc.CENSUS)} rows + {len(excluded)} unreachable")


def test_every_class_has_a_row(union):
    """k_cldr: (scalar type, geometry, GD, GT) with the four epilogue / source forms; k_tile: (scalar type, VEC, TILE_GW, MR);
    k_rows: (scalar type, VEC, GW); both TileSrcFold instances."""
    for S, geoms in (("float", (1, 2, 3, 4)), ("double", (2,))):
        for g in geoms:
            vect, nw, ma, mq, mp = sc.CLDR_GEOMS[g]
            for gd in (6, 8):
                for gt in (12, 16, 24):
                    for epi, src in (("EpiStore", "Plain"), ("EpiCgInit", "Plain"), ("EpiLhs", "Plain"), ("EpiLhs", "Fold")):
                        pat = rf"k_cldr<{S}, {vect}, {epi}<.*>, CldrSrc{src}<.*>, {nw}, {ma}, {mq}, {mp}, {gd}, {gt}, \d>"
                        assert any(re.fullmatch(pat, n) for n in union), pat
    for S, vecs in (("float", (1, 2, 4)), ("double", (1, 2))):
        for v in vecs:
            for gw in (4, 6, 8):
                for mr in (2, 5):
                    assert any(re.fullmatch(rf"k_tile<{S}, {v}, .*, {gw}, {mr}, TileSrcPlain<.*> >", n) for n in union), (S, v, gw, mr)
            for gw in (4, 6):
                assert any(re.fullmatch(rf"k_rows<{S}, {v}, .*, {gw}>", n) for n in union), (S, v, gw)
    assert sum("TileSrcFold" in n for n in union) == 2


def test_ablations_and_tasks_rotate():
    """Every ablation and the mask task under every float32 geometry of k_cldr, and in float64."""
    for dtype, geoms in (("f32", (1, 2, 3, 4)), ("f64", (2,))):
        for g in geoms:
            rows = [r for r in sc.CENSUS if r["name"].startswith(f"cldr-{dtype}-g{g}-")]
            assert {r["abl"] for r in rows} == set(sc.ABLS) and {r["task"] for r in rows} == set(sc.TASKS), (dtype, g)


@pytest.mark.parametrize("r", sc.CENSUS, ids=sc.row_id)
def test_census_graph_has_the_stated_rows(r):
    mu, md, mt, at = sc.row_lengths(r)
    name = r["name"]
    m = re.match(r"cldr-f\d+-g\d-gd(\d+)-gt(\d+)", name)
    if m:
        gd, gt = int(m.group(1)), int(m.group(2))
        assert (md > 6) == (gd == 8) and md <= 8, (md, gd)
        assert {12: 0, 16: 12, 24: 16}[gt] < mt <= gt and r["slots"] == gt, (mt, gt)
    m = re.match(r"tile-f\d+-B\d+-gw(\d)", name)
    if m:
        gw = int(m.group(1))
        assert all((4 if v <= 4 else 6 if v <= 6 else 8) == gw for v in (mu, md)), (mu, md, gw)
        assert (mt <= 4) == (gw == 4)
        if r["graph"][0] == "band" and r["graph"][1].get("hub_in"):
            assert mt > 8                                       # overflow by row length through Ldr_T
    if name == "fallback-k8" or name == "fallback-f64-k8":
        assert md == 9
    if name == "fallback-hub25":
        assert mt == 25 and md <= 8
    if name == "fallback-c2cap":
        assert md <= 6 and 16 < mt <= 24
    if r["graph"][0] == "physical":
        assert mu >= 7                                          # padded rows: the hub of lds_census.physical_graph
    if name.startswith("rows-") and r["graph"][0] == "band":
        k = r["graph"][1]["k"]
        assert (mu, md, at) == ((3, 4, 4) if k == 3 else (6, 7, 7))


def test_tile_rows_cover_the_table_edges():
    """Short last tiles, N < R for both tile sizes, a tile count that is no multiple of 8, halo overflow (scattered columns)."""
    tiles = [r for r in sc.CENSUS if r["tile_rows"]]
    assert any(r["N"] % 8 and r["N"] % 20 for r in tiles)
    assert any(r["N"] < 8 and r["tile_rows"] == 8 for r in tiles) and any(r["N"] < 20 and r["tile_rows"] == 20 for r in tiles)
    assert any(-(-r["N"] // r["tile_rows"]) % 8 for r in tiles)
    for R in (8, 20):
        assert any(r["graph"][0] == "scatter" and r["tile_rows"] == R for r in tiles)
    # a scattered graph of 7 neighbours per row: 8 rows name about 50 distinct out-of-tile rows, far above TILE_HMAX = 20
    cl = sc.scatter_tables(101, 7)[0].numpy()
    assert min(len(set(cl[i:i + 8, 1:].ravel()) - set(range(i, i + 8))) for i in range(0, 96, 8)) > 20


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("cldr") / "cldr_tiles_check")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "cpu", "cldr_tiles_check.cpp"), "-o", exe])
    return exe


def _fused_candidates():
    return [r for r in sc.CENSUS if r["reorder"] and r["graph"][0] in ("band", "scatter") and r["env"].get("MGADMM_FUSED") != "0"]


@pytest.mark.parametrize("r", _fused_candidates(), ids=sc.row_id)
def test_tile_builder_takes_or_refuses_the_graph_as_the_row_states(r, checker, tmp_path):
    """Whether build_cldr_tiles accepts a graph does not depend on the node order (a tile shrinks to a single row before the
    builder gives up), so the natural order decides it here as the cluster order does on the GPU.  The row's `slots` is what
    MGADMM_Q_CLDR_SLOTS must report: 0 where the builder refuses, or where the batch does not fit the chunk width."""
    from mgadmm import utils
    cl, dl = sc.tables_for(r)
    w = utils.directed_graph_from_distance(cl, dl).numpy()
    cl = cl.numpy()
    path = tmp_path / "wd.txt"
    with open(path, "w") as f:
        f.write(f"{cl.shape[0]}\n")
        for i in range(cl.shape[0]):
            keep = cl[i] != -1
            f.write(f"{int(keep.sum())} " + " ".join(f"{c} {v:.9g}" for c, v in zip(cl[i][keep], w[i][keep])) + "\n")
    d = sc.Dispatch(r)
    gd, gt = (8 if d.md > 6 else 6), (12 if d.mt <= 12 else 16 if d.mt <= 16 else 24)
    out = subprocess.run([checker, f"@{path}", str(r["T"]), f"g{d.geom}", str(gd), str(gt), "64"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.match(r"rows max_d (\d+) rows_of_max_d \d+ max_t (\d+)", out.stdout)
    assert m and (int(m.group(1)), int(m.group(2))) == (d.md, d.mt), out.stdout      # the checker saw the census graph
    eligible = out.stdout.strip().endswith("OK")
    assert eligible or out.stdout.strip().endswith("INELIGIBLE"), out.stdout
    fits = d.Bp % (64 * sc.CLDR_GEOMS[d.geom][0]) == 0
    assert r["slots"] == (gt if eligible and fits else 0), (r["name"], out.stdout)


def test_query_items_are_declared():
    from mgadmm import _lib
    assert _lib.Q_STREAM_KEYS == 19 and _lib.Q_STREAM_KEY0 == 1000
    header = open(os.path.join(ROOT, "include", "mgadmm.h")).read()
    assert re.search(r"MGADMM_Q_STREAM_KEYS = 19\b", header) and re.search(r"MGADMM_Q_STREAM_KEY0 = 1000\b", header)
    keys = open(os.path.join(PKG, "csrc", "stream_keys.h")).read()
    names = re.search(r"STREAM_EPI_NAMES\[\] = \{([^}]*)\}", keys).group(1)
    assert tuple(re.findall(r'"(\w+)"', names)) == _lib.STREAM_EPILOGUES
    kern = open(os.path.join(PKG, "csrc", "stream_kernels.h")).read()
    for i, e in enumerate(_lib.STREAM_EPILOGUES):                      # every functor carries the ID of its name
        assert re.search(r"struct %s \{[^\n]*\n    static constexpr int ID = %d;" % (e, i), kern), e
    assert len(re.findall(r"^struct Epi\w+ \{", kern, re.M)) == len(_lib.STREAM_EPILOGUES)


def test_key_decoder():
    """Hand-packed keys (csrc/stream_keys.h): kernel | double << 2 | VEC << 3 | epilogue << 6 | fold << 11 | arguments, 6 bits each
    from bit 12.  Every decoded name is the spelling of a shipped stub."""
    from mgadmm import _lib
    cases = [
        (0 | 0 << 2 | 4 << 3 | 1 << 6 | 6 << 12, "k_rows<float, 4, EpiLhs<float, 4>, 6>"),
        (0 | 1 << 2 | 1 << 3 | 13 << 6 | 4 << 12, "k_rows<double, 1, EpiAddTo<double, 1>, 4>"),
        (1 | 0 << 2 | 4 << 3 | 1 << 6 | 1 << 11 | 4 << 12 | 2 << 18, "k_tile<float, 4, EpiLhs<float, 4>, 4, 2, TileSrcFold<float, 4> >"),
        (1 | 1 << 2 | 2 << 3 | 9 << 6 | 8 << 12 | 5 << 18, "k_tile<double, 2, EpiPhi<double, 2>, 8, 5, TileSrcPlain<double, 2> >"),
        (2 | 1 << 2 | 1 << 3 | 0 << 6 | 8 << 12 | 8 << 18 | 11 << 24 | 15 << 30 | 6 << 36 | 12 << 42 | 2 << 48,
         "k_cldr<double, 1, EpiStore<double, 1>, CldrSrcPlain<double, 1>, 8, 8, 11, 15, 6, 12, 2>"),
        (2 | 4 << 3 | 1 << 6 | 1 << 11 | 16 << 12 | 2 << 18 | 3 << 24 | 4 << 30 | 8 << 36 | 24 << 42 | 4 << 48,
         "k_cldr<float, 4, EpiLhs<float, 4>, CldrSrcFold<float, 4>, 16, 2, 3, 4, 8, 24, 4>"),
    ]
    shipped = shipped_instances()
    for v, name in cases:
        assert _lib.decode_stream_key(v) == name
        assert name in shipped, name


def test_dispatch_model_reads_the_engines_numbers():
    """The geometry table of stream_census.py is parsed from csrc/cldr_tiles.h; the batch thresholds are those of make_geom
    (csrc/stream_plan.h)."""
    assert set(sc.CLDR_GEOMS) == {1, 2, 3, 4} and sc.CLDR_GEOMS[1] == (4, 8, 2, 4, 5)
    assert np.all([sc.vec_of("f32", b)[0] == v for b, v in ((3, 1), (95, 1), (96, 2), (191, 2), (192, 4))])
