"""CPU check of the LDS-tiled row kernel's tables (mixed-graph-admm_amd/csrc/tile_meta.h, plain C++, the builder
Engine::tile_meta uploads): the checker tests/cpu/tile_meta_check.cpp replays k_tile's dataflow on the host from the tables
(own rows and the halo rows the kernel loads in an LDS image, the first TILE_GW local slots, the overflow CSR from the
global vector), compares it with the CSR product to 1e-12 and asserts the invariants the kernel relies on: local indices
inside the rows in use, pad slots = the row itself with weight 0, the halo list a prefix, local + overflow entries = the CSR
row with every entry once, h_rowptr monotone with its padding.  Every case states what it has to exercise; the checker's
statistics line is asserted so that a case cannot quietly stop exercising it."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("tilemeta") / "tile_meta_check")
    # AddressSanitizer + UBSan build of the stand-alone program: an out-of-range index in the builder or the replay aborts
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "cpu", "tile_meta_check.cpp"), "-o", exe])
    return exe


# (n, k, R, GW, kind, perm, hub_indeg, transpose), what the statistics must show
CASES = [
    ((1000, 3, 8, 4, 0, 0, 0, 0), dict(max_row=4, overflow=0)),                       # W_u-like: every row fits its 4 slots
    ((1000, 4, 8, 4, 0, 0, 0, 0), dict(max_row=5, by_length=">0", by_halo=0)),       # rows longer than TILE_GW = 4
    ((1000, 5, 8, 6, 0, 1, 0, 0), dict(max_row=6, by_length=0)),                      # 6 slots, permuted CSR
    ((1003, 6, 8, 6, 0, 0, 0, 0), dict(max_row=7, by_length=">0", last_tile_rows=3)),  # rows longer than TILE_GW = 6, N % 8 != 0
    ((1003, 7, 8, 8, 0, 1, 0, 0), dict(max_row=8, by_length=0, last_tile_rows=3)),    # 8 slots filled exactly
    ((1003, 5, 8, 8, 0, 1, 12, 1), dict(max_row=">8", by_length=">0")),               # transposed: a hub row longer than 8
    ((1003, 4, 20, 4, 0, 0, 0, 0), dict(max_row=5, by_length=">0", last_tile_rows=3)),  # R = 20, N % 20 != 0
    ((1003, 5, 20, 6, 0, 1, 0, 0), dict(max_row=6, last_tile_rows=3)),
    ((1003, 7, 20, 8, 0, 1, 30, 1), dict(max_row=">8", by_length=">0", by_halo=">0", halo_full=">0")),
    ((300, 7, 8, 8, 1, 0, 0, 0), dict(by_length=0, by_halo=">0", halo_full=38)),      # scattered columns: every tile's halo overflows
    ((300, 7, 20, 8, 1, 0, 0, 0), dict(by_length=0, by_halo=">0", halo_full=15)),
    ((1000, 5, 8, 6, 0, 1, 0, 0), dict(halo_full=">0", skipped_batches=">0")),        # full halo lists and waves without a second batch
    ((5, 3, 8, 4, 0, 0, 0, 0), dict(tiles=1, last_tile_rows=5, halo_max=0)),          # N < R
    ((13, 3, 20, 6, 0, 1, 0, 1), dict(tiles=1, last_tile_rows=13, halo_max=0)),       # N < R = 20, transposed
]


@pytest.mark.parametrize("args,expect", CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_tile_tables_reproduce_the_csr_product(checker, args, expect):
    out = subprocess.run([checker] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK"), out.stdout
    stats = {k: float(v) for k, v in re.findall(r"(\w+) ([-+.e\d]+)", out.stdout.splitlines()[0])}
    assert stats["max_err"] <= 1e-12
    # the builder really saw another matrix (the checker permutes clusters of 16 nodes: a graph of one cluster keeps its order)
    assert stats["permuted"] == (1 if args[5] and args[0] > 16 else 0)
    for k, v in expect.items():
        if isinstance(v, str):
            assert stats[k] > float(v[1:]), (k, stats)
        else:
            assert stats[k] == v, (k, stats)


def test_cases_cover_what_the_kernel_can_meet():
    """R in {8, 20} x TILE_GW in {4, 6, 8}, the natural and a permuted node order (the statistics line says whether the
    builder saw another matrix), N < R and N not a multiple of R."""
    assert {(a[2], a[3]) for a, _ in CASES} == {(r, g) for r in (8, 20) for g in (4, 6, 8)}
    assert any(a[5] for a, _ in CASES) and any(not a[5] for a, _ in CASES)
    assert any(a[0] < a[2] for a, _ in CASES) and any(a[0] % a[2] for a, _ in CASES if a[0] > a[2])


def test_the_library_builds_its_tables_with_the_checked_builder():
    """engine.h calls build_tile_meta and keeps no table construction of its own; k_tile's halo capacity is the builder's."""
    eng = open(os.path.join(PKG, "csrc", "engine.h")).read()
    assert "build_tile_meta(A, N, R, TILE_GW, tm)" in eng and "halo_pos" not in eng
    assert "permute_csr(A, perm, iperm, out)" in open(os.path.join(PKG, "csrc", "graph.hip")).read()      # the replayed permutation
    assert '#include "tile_meta.h"' in open(os.path.join(PKG, "csrc", "stream_kernels.h")).read()
    assert len(re.findall(r"constexpr int TILE_HMAX\b", open(os.path.join(PKG, "csrc", "stream_kernels.h")).read()
                          + open(os.path.join(PKG, "csrc", "tile_meta.h")).read())) == 1
