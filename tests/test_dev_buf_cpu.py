"""The owning buffer of the engines' device and pinned memory (mixed-graph-admm_amd/csrc/dev_buf.h, plain C++) on the CPU, and
the conversion of its users.

tests/cpu/dev_buf_check.cpp (built with AddressSanitizer + UBSan, run as a program of its own) instantiates Buf over a
counting policy backed by malloc / free that fails its n-th allocation or copy on request, and checks
  - that no block is alive after any scope (LeakSanitizer backs it up), a move transfers the block and empties its source;
  - reserve: no call below the capacity; a failed growth leaves pointer, capacity and contents, and the next one succeeds;
    a byte count that overflows size_t is refused without a call;
  - upload: a failed copy keeps the old block (none where there was none) and leaks nothing; an empty vector gives one element;
  - reset followed by reserve; a table staged in a local buffer whose later step fails (set_sample_graphs);
  - the set_params sequence that used to record a capacity before its allocations: three buffers at (K1, I1), then (K2, I2)
    with the second allocation failing, then (K2, I2) again.
The failure paths are checked here only: no GPU test injects a failure."""
import json
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

CSRC = os.path.join(PKG, "csrc")
OWNERS = ("engine.h", "lds_engine.h", "graph.hip", "build.hip")


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("devbuf") / "dev_buf_check")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpu", "dev_buf_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads(out.stdout)


def test_the_buffer_check_is_clean_under_asan_and_ubsan(got):
    assert got["live"] == 0 and got["releases"] == got["allocs"] - got["refused"] and got["refused"] >= 5
    assert got["covered_after_failure"] == 1 and got["holds_after_retry"] == 1
    assert got["checks"] >= 60


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_header_is_plain_cpp_and_the_owners_use_it():
    text = _read("dev_buf.h")
    assert [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")] == ["<cstddef>", "<utility>", "<vector>"]
    assert "hip/" not in text and "__global__" not in text and "getenv" not in text
    # nothing is released by hand in the four owners, and nothing is allocated outside the two policies of common.h
    # (frontend.hip keeps its stream-ordered scratch)
    for name in OWNERS:
        src = _read(name)
        for call in ("hipFree(", "hipHostFree(", "hipEventDestroy(", "hipStreamDestroy(", "hipMalloc(", "hipHostMalloc("):
            assert call not in src, (name, call)
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".hip")) and name not in ("common.h", "frontend.hip"):
            assert not re.search(r"\bhip(Host)?Malloc\(", _read(name)), name
    common = _read("common.h")
    assert len(re.findall(r"\bhipMalloc\(", common)) == 1 and len(re.findall(r"\bhipHostMalloc\(", common)) == 1
    policies = common[common.index("struct DevMem"):common.index("template <class T> using DevBuf")]
    assert "hipMalloc(" in policies and "hipHostMalloc(" in policies and "hipFree(" in policies and "hipHostFree(" in policies
    # the capacities that lived beside their pointers are gone
    engines = _read("engine.h") + _read("lds_engine.h")
    for gone in ("max_cg_alloc", "max_admm_alloc", "partials_elems", "hist_ps_elems", "sch_elems", "ad_tab_elems", "ps_full_elems", "free_csr",
                 "auto fr ="):
        assert gone not in engines + _read("graph.hip"), gone
    assert engines.count("alloc_iter_dependent(") == 6      # its definition; init, set_params, cg, solve, two_loops
