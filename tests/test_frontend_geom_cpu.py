"""The launch geometry and the start-index test of the data front end (mixed-graph-admm_amd/csrc/frontend_geom.h, plain
C++) on the CPU.

tests/cpu/frontend_geom_check.cpp (built with AddressSanitizer + UBSan, run as a program of its own) checks
  - window_in_range at 0, n_steps - win, n_steps - win + 1, n_steps, -1, 2^40, INT64_MAX, INT64_MAX - win + 1 and INT64_MIN, and
    against `s0 >= 0 && s0 + win <= n_steps` on small numbers.  The kernel used to form s0 + win, which wraps for a start
    index near 2^63 and then passes; UBSan would end the program on such a sum here;
  - the row chunks of series_stats at 1, 255, 256, 257 steps and at the limit of 65535 chunks +- 1;
  - that every grid covers its range with gridDim.y <= 65535 and without an idle workgroup."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

CSRC = os.path.join(PKG, "csrc")


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("fegeom") / "frontend_geom_check")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpu", "frontend_geom_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads(out.stdout)


def test_the_geometry_check_is_clean_under_asan_and_ubsan(got):
    assert got["max_steps"] == 16776960 == 65535 * 256 and got["max_windows"] == 65535 and got["chunks_at_limit"] == 65535
    assert got["checks"] > 1000


def test_the_header_is_plain_cpp_and_the_kernels_use_it():
    with open(os.path.join(CSRC, "frontend_geom.h")) as f:
        text = f.read()
    assert [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")] == ["<cstdint>", '"mg_hd.h"']
    assert "hip/" not in text and "__global__" not in text and "getenv" not in text
    with open(os.path.join(CSRC, "frontend.hip")) as f:
        hip = f.read()
    # the wrapping sum is gone from the kernel, the refusal precedes the first allocation, the grids come from the header
    assert "s0 + win" not in hip and "fegeom::window_in_range(s0, win, n_steps)" in hip
    body = hip[hip.index("int series_stats("):]
    assert 0 < body.index("fegeom::steps_supported") < body.index("hipMallocAsync")
    for fn in ("stats_chunks", "stats_partials_grid", "stats_finish_grid", "affine_grid", "windows_grid"):
        assert f"fegeom::{fn}(" in hip, fn
