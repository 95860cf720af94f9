"""The launch plan of the streaming path (mixed-graph-admm_amd/csrc/stream_plan.h, plain C++) on the CPU: the launch geometry
of a batch, the kernel instance of every operand class, the fused and fold decisions, and the parsing of the switches.

tests/cpu/stream_plan_check.cpp runs streamplan::Planner on facts and switches given as arguments and prints one JSON object
per case (built with AddressSanitizer + UBSan; it reads no environment).

  * model: for every row of stream_census.CENSUS the keys, the fused flag, the fold flags, VEC and Bp are what the
    independent dispatch model of tests/stream_census.py (Dispatch, vec_of) states -- what tests/test_gpu_stream_census.py
    asserts of the engine on the GPU, here without one;
  * parent: tests/golden/stream_plan_parent.json holds every field of Geom, TileGeom and CldrGeom, the k_cldr geometry in
    force and the slot pair for the cases of parent_cases(), as the rules gave them while they were members of Engine<S>.
    It was made from the text of the commit before the rules moved: make_geom, make_tile_geom, the ClG typedefs with cl_dims,
    make_cldr_geom, cldr_width_fits and the geometry and slot lines of cldr_prepare, cut from `git show` of engine.h by line
    range (with the three records from stream_kernels.h), pasted unchanged into a struct with the members they read, and
    compiled as a host program that read the same case lines and set the switches in its environment.  The rules only
    moved: every field is equal;
  * switches: the clamps and accept rules of Switches::from_strings on literal strings.
"""
import json
import os
import shutil
import subprocess
import sys

import pytest

from conftest import GOLDEN, PKG, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import stream_census as sc      # noqa: E402

PARENT = os.path.join(GOLDEN, "stream_plan_parent.json")
PARENT_FIELDS = ("geom", "tile", "cldr", "cldr_width_fits", "geom_index", "gd", "gt")
OPS = ("none", "band", "lu", "ldr", "ldrt", "ldr+self", "ldrt+self")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stream_plan") / "stream_plan_check")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "cpu", "stream_plan_check.cpp"), "-o", exe])
    return exe


def case_line(elem, T, N, B, mode=0, reorder=2, q1=0, rows=(4, 5, 9, 5), NT=9, **switches):
    """elem T N B mode reorder q1 max_u max_d max_dt avg_dt NT [MGADMM_<SWITCH>=<value> ...]"""
    return " ".join([str(v) for v in (elem, T, N, B, mode, reorder, q1) + tuple(rows) + (NT,)]
                    + [f"MGADMM_{k}={v}" for k, v in switches.items()])


def run_cases(checker, lines, tmp_path):
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([checker, f"@{path}"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    recs = [json.loads(l) for l in out.stdout.splitlines()]
    assert len(recs) == len(lines)
    return recs


# ------------------------------------------------------------------------------------------------ against the model
def census_line(r):
    mu, md, mt, at = sc.row_lengths(r)
    spatial = r["graph"][0] not in ("line", "skip3")
    env = {k[len("MGADMM_"):]: v for k, v in r["env"].items()}
    return case_line(4 if r["dtype"] == "f32" else 8, r["T"], r["N"], r["B"], mode=0 if spatial else 1, reorder=2 if r["reorder"] else 0,
                     rows=(mu, md, mt, at), NT=9 if r["slots"] > 0 else 0, **env)


@pytest.fixture(scope="module")
def census_records(checker, tmp_path_factory):
    return run_cases(checker, [census_line(r) for r in sc.CENSUS], tmp_path_factory.mktemp("census"))


def _named(r, call):
    d = sc.Dispatch(r)
    call(d)
    return d.out


@pytest.mark.parametrize("i", range(len(sc.CENSUS)), ids=[sc.row_id(r) for r in sc.CENSUS])
def test_plan_is_what_the_dispatch_model_states(i, census_records):
    from mgadmm import _lib
    r, got = sc.CENSUS[i], census_records[i]
    d = sc.Dispatch(r)
    assert (got["geom"]["VEC"], got["geom"]["Bp"]) == sc.vec_of(r["dtype"], r["B"]) == (d.VEC, d.Bp)
    for op in OPS:
        assert {_lib.decode_stream_key(got["keys"][op])} == _named(r, lambda m: m.rows("EpiStore", op)), op
    if r["slots"] > 0:                                          # (the model names k_cldr by the row's slot count)
        assert {_lib.decode_stream_key(got["keys"]["cldr"])} == _named(r, lambda m: m.cldr("EpiStore", "Plain"))
        assert got["gt"] == r["slots"]
    assert bool(got["fused"]) == bool(d.fused)
    assert got["tile_rows"] == r["tile_rows"] and got["geom_index"] == d.geom
    # the fold flags of a left-hand side: which folded instance the model's CG solve of that kind launches
    for which in ("x", "zu", "zd"):
        names = _named(r, lambda m: m.cg(which))
        fold1, fold2 = any("CldrSrcFold" in n for n in names), any("TileSrcFold" in n for n in names)
        assert got["fold"][d.kind(which)] == [int(fold1), int(fold2)], (which, names)
    assert got["fold"][0] == [0, 0]


# ------------------------------------------------------------------------------------------------ against the parent
def parent_cases():
    BS = (1, 3, 64, 70, 95, 96, 100, 130, 191, 192, 256, 300, 512, 4096)
    TN = ((4, 7), (4, 13), (12, 96), (4, 101), (12, 131), (24, 307), (24, 883), (12, 10000))
    c = [case_line(e, T, N, B) for e in (4, 8) for B in BS for T, N in TN]
    c += [case_line(e, T, N, B, WANT_BLOCKS=wb) for e in (4, 8) for B in (1, 100, 512, 4096) for T, N in ((4, 7), (12, 131), (12, 10000))
          for wb in (2048, 64)]
    c += [case_line(e, T, N, B, TILE_R=R) for e in (4, 8) for B in (3, 100, 256) for T, N in ((4, 7), (4, 13), (12, 131), (12, 10000)) for R in (8, 20)]
    c += [case_line(e, 12, 10000, B, NT=NT, CLDR_GEOM=g) for e, gs in ((4, (1, 2, 3, 4)), (8, (1, 2))) for g in gs for NT in (1, 9, 1250)
          for B in (70, 100, 256, 300, 512)]
    c += [case_line(e, 12, 131, 256, CLDR_GEOM=g) for e, g in ((8, 3), (8, 4), (4, 0), (4, 5))]                 # values that are not accepted
    c += [case_line(e, 4, 101, 256, rows=(4, md, mt, 5)) for e in (4, 8) for md in (5, 6, 7, 8) for mt in (5, 12, 13, 16, 17, 24)]
    c += [case_line(4, 12, 131, 256, mode=1, rows=(4, 0, 0, 0)), case_line(8, 12, 131, 100, reorder=0), case_line(4, 12, 131, 256, reorder=1),
          case_line(4, 12, 131, 256, TILE=0), case_line(8, 12, 131, 100, TILE=0), case_line(4, 12, 131, 300, q1=1, CLDR_ORDER=0),
          case_line(8, 24, 883, 130, q1=1, CLDR_ORDER=0)]
    return c


def test_rules_give_what_they_gave_inside_the_engine(checker, tmp_path):
    golden = json.load(open(PARENT))
    cases = parent_cases()
    assert [g["args"] for g in golden] == cases and 300 <= len(cases) <= 900
    got = run_cases(checker, cases, tmp_path)
    for g, r in zip(golden, got):
        assert {k: r[k] for k in PARENT_FIELDS} == {k: g[k] for k in PARENT_FIELDS}, g["args"]
    # the grid reaches both sides of every threshold it is there for
    assert {r["geom"]["VEC"] for r in got} == {1, 2, 4} and {r["geom"]["RI"] for r in got} == {4, 8, 12, 16}
    assert {r["tile"]["R"] for r in got if r["tile"]} == {8, 20} and any(r["tile"] is None for r in got)
    assert {(r["gd"], r["gt"]) for r in got} == {(gd, gt) for gd in (6, 8) for gt in (12, 16, 24)}
    assert {r["geom_index"] for r in got} == {1, 2, 3, 4} and {r["cldr_width_fits"] for r in got} == {0, 1}


# ------------------------------------------------------------------------------------------------ the switches
def test_switch_parsing(checker, tmp_path):
    D = dict(want_blocks=2048, tile=1, fused=1, fold=1, fold_lu=1, sweep_rev=1, cldr_tile_major=1, tile_r=8, cldr_geom=0, cldr_rows=0, tile_stats=0)
    cases = [
        (4, {}, {}),
        (4, dict(WANT_BLOCKS="4096"), dict(want_blocks=4096)),
        (4, dict(WANT_BLOCKS="64"), dict(want_blocks=64)),
        (4, dict(WANT_BLOCKS="10"), dict(want_blocks=64)),                     # at least 64
        (4, dict(WANT_BLOCKS="-5"), dict(want_blocks=64)),
        (4, dict(WANT_BLOCKS="many"), dict(want_blocks=64)),                   # (atoi: 0)
        (4, dict(TILE_R="20"), dict(tile_r=20)),
        (4, dict(TILE_R="8"), dict(tile_r=8)),
        (4, dict(TILE_R="12"), dict(tile_r=8)),                                # only 8 or 20
        (4, dict(TILE_R="4"), dict(tile_r=8)),
        (8, dict(TILE_R="20"), dict(tile_r=20)),
        (4, dict(CLDR_GEOM="1"), dict(cldr_geom=1)),
        (4, dict(CLDR_GEOM="3"), dict(cldr_geom=3)),
        (4, dict(CLDR_GEOM="4"), dict(cldr_geom=4)),
        (4, dict(CLDR_GEOM="5"), dict(cldr_geom=0)),                           # 1 .. 4
        (4, dict(CLDR_GEOM="0"), dict(cldr_geom=0)),
        (4, dict(CLDR_GEOM="-1"), dict(cldr_geom=0)),
        (8, dict(CLDR_GEOM="1"), dict(cldr_geom=1)),
        (8, dict(CLDR_GEOM="2"), dict(cldr_geom=2)),
        (8, dict(CLDR_GEOM="3"), dict(cldr_geom=0)),                           # 3 and 4: float only
        (8, dict(CLDR_GEOM="4"), dict(cldr_geom=0)),
        (4, dict(CLDR_ROWS="7"), dict(cldr_rows=7)),
        (4, dict(TILE_STATS="0"), dict(tile_stats=1)),                         # set at all
        (4, dict(TILE="0", FUSED="0", FOLD="0", FOLD_LU="0", SWEEP_REV="0", CLDR_ORDER="0"),
         dict(tile=0, fused=0, fold=0, fold_lu=0, sweep_rev=0, cldr_tile_major=0)),
        (4, dict(TILE="2", FUSED="1"), dict(tile=2)),
        (4, dict(LDS_CHUNK="3", TILE_ROWS="20"), {}),                          # not switches of this path
    ]
    got = run_cases(checker, [case_line(e, 12, 131, 256, **sw) for e, sw, _ in cases], tmp_path)
    for (e, sw, want), r in zip(cases, got):
        assert r["switches"] == dict(D, **want), (e, sw)
    # what the accepted values do: the geometry in force and the tile rows
    assert [r["geom_index"] for r in got[11:21]] == [1, 3, 4, 1, 1, 1, 1, 2, 2, 2]
    assert [r["tile_rows"] for r in got[6:11]] == [20, 8, 8, 8, 20]


def test_plan_header_is_host_only_and_the_engine_reads_no_streaming_switch():
    csrc = os.path.join(PKG, "csrc")
    for h in ("stream_plan.h", "stream_geom.h"):
        text = open(os.path.join(csrc, h)).read()
        assert "hip/" not in text and "__global__" not in text and "__device__" not in text, h
    eng = open(os.path.join(csrc, "engine.h")).read()
    assert [l.split('"')[1] for l in eng.splitlines() if "getenv(" in l] == ["MGADMM_LDS_CHUNK"]
    assert "Switches::from_env" in eng
